"""Prompted LM generation restated in numpy over oracle.roformer's functions: HF GenerationMixin's greedy / sampling loop started from a
decoder prompt (input_ids=), with the processors in HF's order (RepetitionPenalty -> NoRepeatNGram -> Temperature -> TopK -> TopP) over the
WHOLE history, prompt included.  Every row is run alone, cropped to its own phones and prompt -- the definition of the ragged batch
(tests/golden/make_lm_prompt_fixtures.py records the ragged case from the reference that way).  The prompt's tokens but the last only fill
the key/value caches; the last one is the first ordinary step."""
import numpy as np

from oracle import roformer as R

from lm_beam_numpy import ngram_banned

f32 = np.float32


def generate_row(w, cfg, enc, prompt, max_length, do_sample=False, top_k=5, top_p=1.0, temperature=1.0, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, uniforms=None):
    """enc [1,L,hidden] (the row's own encoder states), prompt [P] int (BOS first), uniforms [steps] or None.
    Returns (tokens [n] with the prompt in front, EOS kept; logits [n - P, V]: logits[s] chose the s-th generated token)."""
    prompt = [int(t) for t in prompt]
    if len(prompt) >= max_length:
        raise ValueError(f"the prompt has {len(prompt)} tokens, max_length is {max_length}")
    kv = R.cross_kv(w, cfg, enc)
    caches = [dict() for _ in range(cfg["dec_layers"])]
    for pos, t in enumerate(prompt[:-1]):
        R.decoder_step(w, cfg, np.array([t]), pos, caches, kv)
    seq, out = list(prompt), []
    while len(seq) < max_length:
        lg = R.decoder_step(w, cfg, np.array([seq[-1]]), len(seq) - 1, caches, kv)[0]
        out.append(lg)
        s = lg.astype(f32).copy()
        banned = ngram_banned(seq, no_repeat_ngram_size)
        if not do_sample:
            if repetition_penalty != 1.0:
                for t in set(seq):
                    s[t] = s[t] * f32(repetition_penalty) if s[t] < 0 else s[t] / f32(repetition_penalty)
            for t in banned:
                s[t] = -np.inf
            nxt = int(np.argmax(s))
        else:
            if banned:      # the ban sits between the penalty and the temperature: apply the penalty here, hand pick_token_hf a penalty of 1
                if repetition_penalty != 1.0:
                    for t in set(seq):
                        s[t] = s[t] * f32(repetition_penalty) if s[t] < 0 else s[t] / f32(repetition_penalty)
                for t in banned:
                    s[t] = -np.inf
                nxt = R.pick_token_hf(s, [], top_k, top_p, temperature, 1.0, uniforms[len(out) - 1])
            else:
                nxt = R.pick_token_hf(s, seq, top_k, top_p, temperature, repetition_penalty, uniforms[len(out) - 1])
        seq.append(nxt)
        if nxt == cfg["sem_eos"]:
            break
    return np.array(seq, dtype=np.int64), np.stack(out)


def generate(w, cfg, phone, tone, spk_id, prompt, prompt_len, max_length, enc_len=None, uniforms=None, **kw):
    """the batch as the library defines it: row b = row b alone.  phone / tone / spk_id [B,L], enc_len [B] or None, prompt [B,P],
    prompt_len [B] or None, uniforms [steps,B] or None.  Returns (tokens [B,n] cropped to the longest row, PAD behind the shorter ones;
    a list of the rows' logits)."""
    B = phone.shape[0]
    rows, logits = [], []
    for b in range(B):
        Lb = phone.shape[1] if enc_len is None else int(enc_len[b])
        Pb = prompt.shape[1] if prompt_len is None else int(prompt_len[b])
        enc = R.encoder_forward(w, cfg, phone[b:b + 1, :Lb], tone[b:b + 1, :Lb], None if spk_id is None else spk_id[b:b + 1, :Lb])
        t, lg = generate_row(w, cfg, enc, prompt[b, :Pb], max_length, uniforms=None if uniforms is None else uniforms[:, b], **kw)
        rows.append(t)
        logits.append(lg)
    n = max(len(t) for t in rows)
    toks = np.full((B, n), cfg["sem_pad"], dtype=np.int64)
    for b, t in enumerate(rows):
        toks[b, :len(t)] = t
    return toks, logits
