"""Harness counterpart of the reference's 22_infer_tts.py (22_infer_tts.py:27-114) from the phone / tone ids on:
[phones, tones -> text2semantic RoFormer generate ->] semantic tokens -> unit embeddings (k-means codebook row gather in liblds)
[-> forced alignment] -> DiffusionSVC.infer (Unit2Mel sampler + HiFi-VAEGAN vocoder) -> 44.1 kHz wav.
The grapheme-to-phoneme front end (text/cleaner.py: pypinyin / jieba / g2p tables) is outside this build's scope.

    python infer_tts.py -dm exp/diffusion/model_300000.pt -cb pretrain/semantic_codebook.pt -t tokens.npy -o out.wav
    python infer_tts.py --synthetic -o /tmp/demo.npy        # seeded random weights, synthetic tokens (no checkpoints exist)
    python infer_tts.py ... -lm exp/lm/model.pt -p phones.npy --prompt_tokens ref_tokens.npy --prompt_phones ref_phones.npy
                                                            # continue a voice / prosody prompt: the waveform is the continuation only
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "latent-diffusion-speech_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-dm", "--diffusion_model")
    ap.add_argument("-cb", "--codebook", help="semantic_codebook.pt: the reference's KMeans dict (cluster/__init__.py:5-11) or a plain [n_codes, dim] tensor")
    ap.add_argument("-t", "--tokens", help=".npy int array [T] of semantic token ids")
    ap.add_argument("-lm", "--language_model", help="exp/lm/model_<step>.pt ({'model': Roformer.state_dict()}) with config.yaml next to it")
    ap.add_argument("-p", "--phones", help=".npy int array [2, L]: phone ids and tone ids (text_to_sequence output); tokens come from the LM")
    ap.add_argument("--max_length", type=int, default=1024)
    ap.add_argument("--num_beams", type=int, default=1, help="> 1: greedy beam search over the semantic tokens instead of top-k sampling (2 .. 8)")
    ap.add_argument("--no_repeat_ngram_size", type=int, default=0, help="n >= 1: no n-gram of semantic tokens repeats (HF NoRepeatNGramLogitsProcessor)")
    ap.add_argument("--candidates", type=int, default=1,
                    help="N > 1: sample N token sequences in one batch, score them with the LM (Roformer.score / Llama.score) and keep the one with the highest mean "
                         "log-prob per generated token (sampling only: num_beams 1)")
    ap.add_argument("--prompt_tokens", help=".npy int array [Tp] of semantic token ids the LM continues from (BOS is added): a voice / prosody prompt, or "
                                            "the tail of the previous sentence")
    ap.add_argument("--prompt_phones", help=".npy int array [2, Lp]: the prompt's own phone and tone ids, put in front of --phones")
    ap.add_argument("--prompt_audio", help="a clip (.wav PCM16 or .npy at --prompt_sample_rate) whose semantic tokens become the prompt: resampler -> "
                                           "units encoder -> nearest codebook centre, as tools/extract_tokens.py --from-audio")
    ap.add_argument("--prompt_sample_rate", type=int, default=16000)
    ap.add_argument("--prompt_encoder", default="whisper_large_v3", choices=("whisper_large_v3", "hubertsoft", "contentvec768l12", "w2v-bert"))
    ap.add_argument("--prompt_encoder_checkpoint", default=None)
    ap.add_argument("--prompt_encoder_layers", type=int, default=None, help="depth of the seeded units encoder that --synthetic uses for --prompt_audio")
    ap.add_argument("--keep_prompt", action="store_true", help="synthesise the prompt's tokens too (default: the continuation only)")
    ap.add_argument("-o", "--output", default="output.npy")
    ap.add_argument("-id", "--spk_id", type=int, default=1)
    ap.add_argument("-s", "--speedup", type=int, default=10)
    ap.add_argument("-me", "--method", default="dpm-solver")
    ap.add_argument("--scale_factor", type=float, default=None,
                    help="nearest-resample the unit frames by this factor first (22_infer_tts.py:108-110, units_forced_alignment)")
    ap.add_argument("--latency_mode", action="store_true",
                    help="one sentence per call: tile shapes / reduction splits from the actual batch (include/lds.h lds_unet_set_latency_mode)")
    ap.add_argument("--gemm_mode", default="f32", choices=["f32", "split_f16"], help="the UNet's GEMMs (include/lds.h lds_unet_set_gemm_mode)")
    ap.add_argument("--lm_type", default="roformer", choices=("roformer", "llama"),
                    help="which seeded LM --synthetic builds: the RoFormer encoder / decoder or the decoder-only Llama (a checkpoint's config.yaml names its own)")
    ap.add_argument("--index", help="units_index.pt (tools/train_units_index.py): the codebook centres of the tokens are blended with their nearest "
                                    "rows of this pool of the speaker's units before the alignment (units retrieval, exact and on the device)")
    ap.add_argument("--index_ratio", type=float, default=0.5, help="0 .. 1: the share of the retrieved units in the blend")
    ap.add_argument("--index_k", type=int, default=8, help="1 .. 8 nearest pool rows per frame")
    ap.add_argument("--index_nprobe", type=int, default=None, help="1 .. 8: search only the rows of a frame's N best lists (an index written with --nlist)")
    ap.add_argument("--index_weights", default="inverse_square", choices=("inverse_square", "uniform"),
                    help="the blend's weights: 1 / d^2 over the distances, or the plain mean of the rows found (the metric comes from the index file)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--synthetic_tokens", type=int, default=256)
    return ap.parse_args(argv)


def synthetic_pipeline(dev, n_tokens):
    """seeded random-init model, vocoder, codebook and tokens (no checkpoints ship with the reference)"""
    from diffusion.unit2mel import Unit2Mel
    from diffusion.vocoder import Vocoder
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch, init_weights
    from tools.infer_tools import DiffusionSVC
    h = arch.SYNTHETIC_VOCODER_H
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder = Hifi_VAEGAN(None, device=dev, h=h, state=init_weights.init_state(arch.generator_param_shapes(h), 0))
    voc.vocoder_hop_size, voc.vocoder_sample_rate, voc.dimension, voc.device = h["hop_size"], h["sampling_rate"], h["inter_channels"], dev
    svc = DiffusionSVC(device=dev)
    svc.model, svc.vocoder = Unit2Mel(1280, 323, 80).to(dev).eval(), voc
    codebook = torch.from_numpy(init_weights.uniform("synthetic.codebook", (4096, 1280), 5, -1.7, 1.7)).to(dev)
    tokens = torch.from_numpy((np.arange(n_tokens) * 131 % 4096).astype(np.int64)).to(dev)
    return svc, codebook, tokens


def load_codebook(path, dev):
    from cluster import codebook_to_device, get_cluster_model
    try:
        return codebook_to_device(get_cluster_model(path), dev)              # the reference's on-disk format
    except (KeyError, TypeError, IndexError):
        return torch.load(path, map_location=dev).float().contiguous()     # a bare centre matrix


def synthetic_lm(dev):
    """seeded random-init text2semantic model in the reference's phone-mode configuration"""
    from lds import arch
    from text2semantic.roformer.roformer import Roformer
    c = arch.roformer_config()
    hf = dict(hidden_size=c["hidden"], num_attention_heads=c["heads"], intermediate_size=c["inter"], hidden_act="gelu",
              max_position_embeddings=c["max_pos"], layer_norm_eps=c["eps"])
    return Roformer(dict(hf, num_hidden_layers=c["enc_layers"]), dict(hf, num_hidden_layers=c["dec_layers"]), mode="phone",
                    semantic_kmeans_num=c["semantic_kmeans_num"], codebook_path="", n_spk=c["n_spk"]).to(dev).eval()


def synthetic_llama(dev):
    """seeded random-init decoder-only text2semantic model: the width of the reference's own example (llama.py:186-193: hidden 768, 4 heads,
    4 layers, intermediate 512) over the synthetic codebook's 4096 tokens"""
    from text2semantic.llama.llama import Llama
    return Llama(dict(hidden_size=768, num_attention_heads=4, num_hidden_layers=4, intermediate_size=512, max_position_embeddings=2048),
                 mode="phone", semantic_kmeans_num=4096, codebook_path="").to(dev).eval()


def load_lm(path, dev):
    import yaml
    from text2semantic.utils import get_language_model
    args = yaml.safe_load(open(os.path.join(os.path.split(path)[0], "config.yaml")))
    lm = get_language_model(**args).to(dev)
    lm.load_state_dict(torch.load(path, map_location=torch.device(dev))["model"])
    return lm.eval()


def with_bos(lm, prompt_tokens, rows=1):
    """semantic ids [Tp] -> the decoder prompt [rows, 1 + Tp] that Roformer.generate and Llama.generate take (BOS first)"""
    bos = lm.config.bos_token_id - lm.semantic_token_shift if hasattr(lm, "llama") else lm.semantic_bos_token_id      # (the Llama's K, in returned numbering)
    p = torch.cat([prompt_tokens.new_full((1,), bos), prompt_tokens.reshape(-1)])
    return p[None].expand(rows, -1).contiguous()


def tokens_from_audio(a, codebook, dev):
    """--prompt_audio: the clip's semantic tokens through the functions tools/extract_tokens.py --from-audio uses (everything on the device)"""
    import types
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from extract_tokens import units_encoder
    from extract_units import encoder_batch, load_clip
    ue = units_encoder(types.SimpleNamespace(encoder=a.prompt_encoder, synthetic_encoder=a.synthetic, checkpoint=a.prompt_encoder_checkpoint,
                                             layers=a.prompt_encoder_layers, seed=0))
    audio, slen = encoder_batch([load_clip(a.prompt_audio, a.prompt_sample_rate)], ue.min_samples)
    model = types.SimpleNamespace(cluster_centers_=codebook.detach().cpu().numpy())
    tok, lens = ue.encode_tokens_ragged(audio, slen, model, pad_id=-1)
    return tok[0, : int(lens[0])].to(device=dev, dtype=torch.int64)


def text2semantic(lm, phones, tones, spk_id=1, max_length=1024, num_beams=1, no_repeat_ngram_size=0, semantic_prompt=None, keep_prompt=False):
    """22_infer_tts.py:76-104: sample the semantic tokens (top-k 5, temperature 1) and strip BOS / EOS.  phones, tones [B,L] int64.
    num_beams > 1: greedy beam search instead of sampling; no_repeat_ngram_size n >= 1: no n-gram repeats (either decode).
    semantic_prompt [B,P] (BOS first): the decode continues it; its tokens are stripped with BOS unless keep_prompt."""
    spk = torch.ones_like(phones) * spk_id
    P = 1 if semantic_prompt is None else semantic_prompt.shape[1]      # ids in front of the generated ones: BOS, or the prompt (BOS first)
    first = 1 if keep_prompt else P
    tok = lm.generate(phones, tones, attention_mask=None, use_cache=None, max_length=max_length, do_sample=num_beams == 1, temperature=1.0, top_k=5,
                      top_p=1.0, repetition_penalty=1.0, num_beams=num_beams, no_repeat_ngram_size=no_repeat_ngram_size, early_stopping=True, spk_id=spk,
                      end_gate_threshold=None, **({} if semantic_prompt is None else {"semantic_prompt": semantic_prompt}))
    # reference 22_infer_tts.py:100-103 (`if semantic_token[:, -1] == eos`: written for one utterance; on a batch that line itself raises).
    # The batched counterpart: every row ending with its EOS at the same step is stripped like the single row; rows that all ran to max_length
    # come back whole; rows that ended at DIFFERENT steps (EOS / PAD ids inside the result) cannot be one rectangular tensor.
    eos = lm.semantic_eos_token_id
    body_has_stop = bool((tok[:, P:-1] >= eos).any()) if tok.shape[1] > P + 1 else False
    if not body_has_stop and bool((tok[:, -1] == eos).all()):
        return tok[:, first:-1]
    if body_has_stop or bool((tok[:, -1] >= eos).any()):
        raise ValueError("rows of a batch ended at different lengths (EOS / PAD ids in the result): use text2semantic_rows, which cuts every "
                         "row at its own EOS, and synthesize_ragged")
    return tok[:, first:]


def text2semantic_llama(lm, phones, tones, spk_id=1, max_length=1024, no_repeat_ngram_size=0, semantic_prompt=None, keep_prompt=False):
    """`text2semantic` for the decoder-only Llama (reference llama.py:121-184): its generate returns the ids behind the semantic BOS alone (no BOS
    in front, the shift subtracted); max_length counts the L + 3 prompt ids and the prompt's tokens.  One utterance: phones, tones [1, L].
    semantic_prompt [1,P] (BOS first): the decode continues it; its P - 1 tokens are stripped unless keep_prompt."""
    tok = lm.generate(phones, tones, attention_mask=None, use_cache=None, max_length=max_length, do_sample=True, temperature=1.0, top_k=5, top_p=1.0,
                      repetition_penalty=1.0, num_beams=1, no_repeat_ngram_size=no_repeat_ngram_size, early_stopping=True,
                      spk_id=torch.ones_like(phones) * spk_id, end_gate_threshold=None,
                      **({} if semantic_prompt is None else {"semantic_prompt": semantic_prompt}))
    eos = lm.config.eos_token_id - lm.semantic_token_shift
    first = 0 if keep_prompt or semantic_prompt is None else semantic_prompt.shape[1] - 1
    return tok[:, first:-1] if bool((tok[:, -1] == eos).all()) else tok[:, first:]


def text2semantic_llama_candidates(lm, phones, tones, spk_id=1, max_length=1024, candidates=2, no_repeat_ngram_size=0, semantic_prompt=None,
                                   keep_prompt=False):
    """text2semantic_llama for one utterance with N sampled candidates decoded as one batch and ranked with ONE Llama.score call: the row with the
    highest mean log-prob per generated token (over the full vocabulary, a row counting up to and including its EOS) comes back as [1, n], cut
    before its EOS.  semantic_prompt [1,P] (BOS first): every candidate continues it, its tokens are labelled -100 so that only the continuation
    is counted, and they are stripped unless keep_prompt."""
    if phones.shape[0] != 1:
        raise ValueError("candidates are drawn for one utterance at a time (phones [1, L])")
    ph, tn = phones.expand(candidates, -1).contiguous(), tones.expand(candidates, -1).contiguous()
    tok = lm.generate(ph, tn, attention_mask=None, use_cache=None, max_length=max_length, do_sample=True, temperature=1.0, top_k=5, top_p=1.0,
                      repetition_penalty=1.0, num_beams=1, no_repeat_ngram_size=no_repeat_ngram_size, early_stopping=True, spk_id=torch.ones_like(ph) * spk_id,
                      end_gate_threshold=None, **({} if semantic_prompt is None else {"semantic_prompt": semantic_prompt.expand(candidates, -1).contiguous()}))
    n_prompt = 0 if semantic_prompt is None else semantic_prompt.shape[1] - 1
    eos = lm.config.eos_token_id - lm.semantic_token_shift
    # a row's length: up to and including its first EOS behind the prompt (an EOS or pad id inside the prompt must not end the row)
    stop = tok[:, n_prompt:] == eos
    length = torch.where(stop.any(1), stop.int().argmax(1) + 1 + n_prompt, torch.full_like(tok[:, 0], tok.shape[1]))
    mask = (torch.arange(tok.shape[1], device=tok.device)[None] < length[:, None]).to(torch.int64)
    labels = tok.clone()
    labels[:, :n_prompt] = -100
    r = lm.score(ph, tn, tok, semantic_attention_mask=mask, labels=labels)
    mean_lp = r.seq_logprob / r.ranks.ge(0).sum(1)
    best = int(mean_lp.argmax())
    print(f"candidates: mean log-prob per token {[round(float(v), 4) for v in mean_lp]}, kept {best}")
    end = int(length[best]) - (1 if bool(stop[best].any()) else 0)
    return tok[best][None, 0 if keep_prompt else n_prompt: end]


def pick_candidate(lm, phones, tones, tok, spk_id=1, prompt_len=1):
    """Rank N sampled sequences of ONE utterance with one Roformer.score call.  phones, tones [1,L]; tok [N,n] as generate returns it (BOS, the
    tokens, then EOS and PAD in rows that finished early: a row counts up to and including its EOS).  Returns (index of the row with the highest
    mean log-prob per generated token, those means [N], the LMScore).  prompt_len > 1: the first prompt_len ids of every row are a given prompt
    (BOS included); they are labelled -100, so only the continuation is counted."""
    N, n = tok.shape
    stop = tok[:, 1:] == lm.semantic_eos_token_id
    length = torch.where(stop.any(1), stop.int().argmax(1) + 2, torch.full_like(tok[:, 0], n))
    mask = (torch.arange(n, device=tok.device)[None] < length[:, None]).to(torch.int64)
    ph, tn = phones.expand(N, -1).contiguous(), tones.expand(N, -1).contiguous()
    labels = None
    if prompt_len > 1:
        labels = tok.clone()
        labels[:, :prompt_len] = -100
    r = lm.score(ph, tn, tok, attention_mask=mask, labels=labels, spk_id=torch.ones_like(ph) * spk_id)
    mean_lp = r.seq_logprob / r.ranks.ge(0).sum(1)
    return int(mean_lp.argmax()), mean_lp, r


def text2semantic_candidates(lm, phones, tones, spk_id=1, max_length=1024, candidates=2, no_repeat_ngram_size=0, semantic_prompt=None, keep_prompt=False):
    """text2semantic for one utterance with N sampled candidates decoded as one batch; the best one under the LM (pick_candidate) comes back as
    [1, n]: BOS stripped, cut before its EOS.  semantic_prompt [1,P] (BOS first): every candidate continues it, the ranking counts the
    continuation only, and the prompt is stripped with BOS unless keep_prompt."""
    if phones.shape[0] != 1:
        raise ValueError("candidates are drawn for one utterance at a time (phones [1, L])")
    ph, tn = phones.expand(candidates, -1).contiguous(), tones.expand(candidates, -1).contiguous()
    tok = lm.generate(ph, tn, attention_mask=None, use_cache=None, max_length=max_length, do_sample=True, temperature=1.0, top_k=5, top_p=1.0,
                      repetition_penalty=1.0, num_beams=1, no_repeat_ngram_size=no_repeat_ngram_size, early_stopping=True, spk_id=torch.ones_like(ph) * spk_id,
                      end_gate_threshold=None, **({} if semantic_prompt is None else {"semantic_prompt": semantic_prompt.expand(candidates, -1).contiguous()}))
    P = 1 if semantic_prompt is None else semantic_prompt.shape[1]
    best, mean_lp, _ = pick_candidate(lm, phones, tones, tok, spk_id, prompt_len=P)
    row = tok[best]
    stop = (row[P:] >= lm.semantic_eos_token_id).nonzero()
    print(f"candidates: mean log-prob per token {[round(float(v), 4) for v in mean_lp]}, kept {best}")
    return row[None, 1 if keep_prompt else P: P + int(stop[0]) if stop.numel() else row.shape[0]]


def text2semantic_rows(lm, phones, tones, spk_id=1, max_length=1024, phone_lengths=None, num_beams=1, no_repeat_ngram_size=0, prompt_rows=None,
                       keep_prompt=False):
    """A batch of sentences of DIFFERENT lengths (BASELINE configs[4]: 64 sentences per call).  phones / tones [B,L] right-padded,
    phone_lengths [B] (None = all L): the padding mask goes through the encoder and the cross-attention (reference roformer.py:209-236).
    Returns one 1-D token tensor per row: BOS stripped, cut before the row's first EOS (rows that finish early are padded by generate;
    the ids EOS = kmeans_num + 1 and PAD = kmeans_num + 2 have no codebook row and must never reach the unit lookup).  num_beams and
    no_repeat_ngram_size as in text2semantic.  prompt_rows: one 1-D tensor of semantic ids per row (empty or None: no prompt; BOS is added):
    every row continues its own prompt as if it ran alone, and comes back without it unless keep_prompt."""
    B, L = phones.shape
    mask = None
    if phone_lengths is not None:
        mask = (torch.arange(L, device=phones.device)[None] < torch.as_tensor(phone_lengths, device=phones.device)[:, None]).to(torch.int64)
    spk = torch.ones_like(phones) * spk_id
    plen, extra = [1] * B, {}
    if prompt_rows is not None:
        plen = [1 + (0 if r is None else int(r.numel())) for r in prompt_rows]
        prompt = torch.full((B, max(plen)), lm.semantic_pad_token_id, dtype=torch.int64, device=phones.device)
        prompt[:, 0] = lm.semantic_bos_token_id
        for b, r in enumerate(prompt_rows):
            if plen[b] > 1:
                prompt[b, 1:plen[b]] = r.to(phones.device)
        pmask = (torch.arange(prompt.shape[1], device=phones.device)[None] < torch.as_tensor(plen, device=phones.device)[:, None]).to(torch.int64)
        extra = dict(semantic_prompt=prompt, prompt_attention_mask=pmask)
    tok = lm.generate(phones, tones, attention_mask=mask, use_cache=None, max_length=max_length, do_sample=num_beams == 1, temperature=1.0, top_k=5,
                      top_p=1.0, repetition_penalty=1.0, num_beams=num_beams, no_repeat_ngram_size=no_repeat_ngram_size, early_stopping=True, spk_id=spk,
                      end_gate_threshold=None, **extra)
    tok = tok.cpu()
    rows = []
    for b in range(B):
        stop = (tok[b, plen[b]:] >= lm.semantic_eos_token_id).nonzero()
        n = plen[b] + int(stop[0]) if stop.numel() else tok.shape[1]
        rows.append(tok[b, 1 if keep_prompt else plen[b]: n].to(phones.device))
    return rows


_STREAM_POOLS = {}


def _stream_pool(dev, n):
    """n side streams per device, created once: every (handle, stream) pair owns a workspace (lds/native.py Workspace), so the streams
    are reused across calls instead of drawn anew"""
    key = str(torch.device(dev))
    pool = _STREAM_POOLS.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(dev))
    return pool[:n]


def synthesize_ragged_masked(svc, codebook, token_rows, spk_id=1, speedup=10, method="dpm-solver", noise_fn=None, streams=1, max_batch=16,
                             ragged_vocoder=True):
    """Utterances of different lengths with the SAMPLER run as one padded batch per `max_batch` rows and per-utterance lengths inside the
    kernels (Unit2Mel.forward_ragged: every utterance as if it ran alone -- statistics, attention and resampling stop at its own length;
    within the parity tolerances of the stand-alone run, not bit for bit), then the vocoder on the same padded batch (ragged_vocoder, the
    default: lds_vocoder_forward_ragged) or per length bucket on `streams` HIP streams.
    Rows are sorted by length so that a padded batch wastes few frames.  Returns [(mel [T,M], wav [T*hop])] in the order of `token_rows`."""
    from lds import native
    order = sorted((i for i, r in enumerate(token_rows) if r.numel() > 0), key=lambda i: -int(token_rows[i].numel()))
    mels = [None] * len(token_rows)
    wavs = [None] * len(token_rows)
    for c0 in range(0, len(order), max_batch):
        idx = order[c0:c0 + max_batch]
        lens = [int(token_rows[i].numel()) for i in idx]
        T = max(lens)
        tok = torch.zeros(len(idx), T, dtype=torch.int64, device=codebook.device)
        for j, i in enumerate(idx):
            tok[j, :lens[j]] = token_rows[i]
        units = native.gather_rows(codebook, tok)
        xT = None
        if noise_fn is not None:      # the start noise handed down explicitly (GaussianDiffusion.forward's x_T), every row at its own length
            xT = torch.zeros(len(idx), 1, svc.model.decoder.out_dims, T, device=codebook.device)
            for j, i in enumerate(idx):
                xT[j:j + 1, :, :, :lens[j]] = noise_fn([i], lens[j])
        mel = svc.call_ragged(units, lens, spk_id=spk_id, infer_speedup=speedup, method=method, x_T=xT)
        if ragged_vocoder:      # ... and the vocoder on the same padded batch, every stage masked at the utterance's up-sampled length
            wav = svc.vocoder.infer_ragged(mel, lens)
            hop = wav.shape[-1] // T
            for j, i in enumerate(idx):
                wavs[i] = wav[j, 0, :lens[j] * hop].contiguous()
        for j, i in enumerate(idx):
            mels[i] = mel[j, :lens[j]].contiguous()
    if ragged_vocoder:
        return [(mels[i], wavs[i]) if token_rows[i].numel() else (torch.empty(0, svc.model.decoder.out_dims), torch.empty(0)) for i in range(len(token_rows))]
    # ragged_vocoder = False: the vocoder per length bucket (bit-identical with each mel decoded alone)
    out = [None] * len(token_rows)
    by_len = {}
    for i, r in enumerate(token_rows):
        by_len.setdefault(int(r.numel()), []).append(i)

    def voc_bucket(T, idx):
        if T == 0:
            for i in idx:
                out[i] = (torch.empty(0, svc.model.decoder.out_dims), torch.empty(0))
            return
        wav = svc.mel2wav(torch.stack([mels[i] for i in idx]), None)
        for j, i in enumerate(idx):
            out[i] = (mels[i], wav[j, 0])
    buckets = sorted(by_len.items())
    if streams <= 1 or len(buckets) <= 1:
        for T, idx in buckets:
            voc_bucket(T, idx)
        return out
    dev = codebook.device
    cur = torch.cuda.current_stream(dev)
    pool = _stream_pool(dev, min(streams, len(buckets)))
    for k, s_ in enumerate(pool):
        s_.wait_stream(cur)
        with torch.cuda.stream(s_):
            for T, idx in buckets[k::len(pool)]:
                voc_bucket(T, idx)
    for s_ in pool:
        cur.wait_stream(s_)
    for mel_wav in out:
        for t in mel_wav:
            if t.is_cuda:
                t.record_stream(cur)
    return out


def synthesize_ragged(svc, codebook, token_rows, spk_id=1, speedup=10, method="dpm-solver", noise_fn=None, streams=1):
    """Utterances of different lengths through the sampler and the vocoder: rows of equal length run as one batch, and because no kernel
    reduces across the batch axis (batch invariance) every utterance's mel / waveform is bit-identical to running it alone.
    token_rows: list of 1-D int64 tensors.  noise_fn(n_utt, T) -> x_T [n_utt,1,M,T] injects the start noise (tests); returns a list of
    (mel [T,M], wav [T*hop]) in the order of `token_rows`.
    streams > 1: the length buckets are spread over that many HIP streams (each with its own workspace, lds/native.py Workspace) and, unless
    noise_fn is given, over as many host threads -- ctypes releases the GIL while a sampler call enqueues its ~12 k launches.  A bucket of
    one or two utterances leaves most of the chip idle, so buckets overlap on the GPU; the results are the same tensors either way."""
    from lds import native
    out = [None] * len(token_rows)
    by_len = {}
    for i, r in enumerate(token_rows):
        by_len.setdefault(int(r.numel()), []).append(i)

    def run_bucket(T, idx):
        if T == 0:
            for i in idx:
                out[i] = (torch.empty(0, svc.model.decoder.out_dims), torch.empty(0))
            return
        tok = torch.stack([token_rows[i] for i in idx])
        units = native.gather_rows(codebook, tok)
        xT = noise_fn(idx, T) if noise_fn is not None else None
        mel = svc(units, f0=None, volume=None, spk_id=spk_id, infer_speedup=speedup, method=method, x_T=xT)
        wav = svc.mel2wav(mel, None)
        for j, i in enumerate(idx):
            out[i] = (mel[j], wav[j, 0])

    buckets = sorted(by_len.items(), key=lambda kv: -kv[0] * len(kv[1]))      # largest first
    if streams <= 1 or len(buckets) <= 1:
        for T, idx in sorted(by_len.items()):
            run_bucket(T, idx)
        return out
    dev = codebook.device
    cur = torch.cuda.current_stream(dev)
    pool = _stream_pool(dev, min(streams, len(buckets)))
    for s_ in pool:
        s_.wait_stream(cur)      # the inputs were produced on the caller's stream

    with torch.cuda.stream(pool[0]):      # the first bucket on this thread: it creates whatever native handle does not exist yet
        run_bucket(*buckets[0])
    buckets = buckets[1:]

    def worker(k):
        with torch.cuda.stream(pool[k]):
            for T, idx in buckets[k::len(pool)]:
                run_bucket(T, idx)
    import threading
    ths = [threading.Thread(target=worker, args=(k,)) for k in range(len(pool))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for s_ in pool:
        cur.wait_stream(s_)
    for mel_wav in out:      # the caller's stream owns the results from here on
        for t in mel_wav:
            if t.is_cuda:
                t.record_stream(cur)
    return out


def synthesize(svc, codebook, tokens, spk_id=1, speedup=10, method="dpm-solver", scale_factor=None, *, index=None, index_ratio=0.5, index_k=8, index_nprobe=None,
               index_weights="inverse_square"):
    """tokens [T] (or [B,T]) int64 on the device -> (units [B,T',C], mel [B,T',M], wav [B,1,T'*hop]); index (cluster.index.UnitsIndex): the
    gathered centres are blended with their index_k nearest pool rows at index_ratio before the alignment (index_nprobe: through the index's IVF)"""
    from lds import native
    from tools.tools import units_forced_alignment
    tok = tokens if tokens.dim() == 2 else tokens[None]
    units = native.gather_rows(codebook, tok)                                  # semantic_embedding(semantic_token), 22_infer_tts.py:106
    if index is not None:
        units = index.retrieve(units, k=index_k, ratio=index_ratio, nprobe=index_nprobe, weights=index_weights)
    if scale_factor is not None:
        units = units_forced_alignment(units, scale_factor=scale_factor)
    mel = svc(units, f0=None, volume=None, spk_id=spk_id, infer_speedup=speedup, method=method)
    wav = svc.mel2wav(mel, None)
    return units, mel, wav


def main(argv=None):
    a = parse_args(argv)
    if not a.phones and (a.prompt_tokens or a.prompt_phones or a.prompt_audio or a.keep_prompt):
        raise SystemExit("--prompt_tokens / --prompt_phones / --prompt_audio / --keep_prompt prompt the LM: they need --phones")
    dev = "cuda"
    lm = None
    if a.synthetic:
        svc, codebook, tokens = synthetic_pipeline(dev, a.synthetic_tokens)
        if a.phones:
            lm = synthetic_llama(dev) if a.lm_type == "llama" else synthetic_lm(dev)
    else:
        from tools.infer_tools import DiffusionSVC
        svc = DiffusionSVC(device=dev)
        svc.load_model(a.diffusion_model)
        codebook = load_codebook(a.codebook, dev)
        tokens = torch.from_numpy(np.load(a.tokens).astype(np.int64)).to(dev) if a.tokens else None
        if a.language_model:
            lm = load_lm(a.language_model, dev)
    svc.model.decoder.denoise_fn.set_gemm_mode(a.gemm_mode)
    svc.model.decoder.denoise_fn.set_latency_mode(a.latency_mode)
    if a.phones:
        if lm is None:
            raise SystemExit("--phones needs --language_model (or --synthetic)")
        pt = torch.from_numpy(np.load(a.phones).astype(np.int64)).to(dev)
        if a.candidates < 1 or (a.candidates > 1 and a.num_beams != 1):
            raise SystemExit("--candidates needs N >= 1 and, for N > 1, sampling (--num_beams 1)")
        prompt = {}
        if hasattr(lm, "llama") and a.num_beams > 1:
            raise SystemExit("beam search is not built for the Llama LM: --num_beams is the RoFormer's (prompts and --candidates work with both)")
        if a.prompt_tokens and a.prompt_audio:
            raise SystemExit("--prompt_tokens and --prompt_audio both name the prompt: give one")
        if a.prompt_phones:
            pt = torch.cat([torch.from_numpy(np.load(a.prompt_phones).astype(np.int64)).to(dev), pt], dim=1)
        if a.prompt_tokens or a.prompt_audio:
            ptok = torch.from_numpy(np.load(a.prompt_tokens).astype(np.int64)).to(dev) if a.prompt_tokens else tokens_from_audio(a, codebook, dev)
            prompt = dict(semantic_prompt=with_bos(lm, ptok), keep_prompt=a.keep_prompt)
        if hasattr(lm, "llama"):      # the decoder-only LM: sampling, optionally from a prompt and with ranked candidates
            fn = text2semantic_llama if a.candidates == 1 else text2semantic_llama_candidates
            tokens = fn(lm, pt[0:1], pt[1:2], a.spk_id, a.max_length, **({} if a.candidates == 1 else {"candidates": a.candidates}),
                        no_repeat_ngram_size=a.no_repeat_ngram_size, **prompt)
        elif a.candidates > 1:
            tokens = text2semantic_candidates(lm, pt[0:1], pt[1:2], a.spk_id, a.max_length, a.candidates, a.no_repeat_ngram_size, **prompt)
        else:
            tokens = text2semantic(lm, pt[0:1], pt[1:2], a.spk_id, a.max_length, a.num_beams, a.no_repeat_ngram_size, **prompt)
        tokens = tokens.clamp(max=codebook.shape[0] - 1)      # pad ids of finished rows (batch > 1) have no codebook row
    index = None
    if a.index:
        from cluster.index import UnitsIndex
        index = UnitsIndex.load(a.index)
    _, _, wav = synthesize(svc, codebook, tokens, a.spk_id, a.speedup, a.method, a.scale_factor, index=index, index_ratio=a.index_ratio, index_k=a.index_k,
                           index_nprobe=a.index_nprobe, index_weights=a.index_weights)
    wav = wav[0, 0].cpu().numpy()
    if a.output.endswith(".wav"):
        import wave
        with wave.open(a.output, "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(44100)
            f.writeframes((np.clip(wav, -1, 1) * 32767).astype("<i2").tobytes())
    else:
        np.save(a.output, wav)
    print(f"wrote {a.output}: {wav.shape[0]} samples ({wav.shape[0] / 44100:.2f} s)")
    return wav


if __name__ == "__main__":
    main()
