"""The validation pass of a text2semantic checkpoint (the reference's text2semantic/roformer/train.py:15-71 `test`, without the audio
logging): for every item the teacher-forced loss of its semantic tokens and the top-5 accuracy of the next-token prediction, then their
means over the items -- Roformer.score in place of the reference's model(**data) (.loss, get_topk_acc(..., k=5)).

    python tools/validate_lm.py --model exp/lm/model_100000.pt --data VALID_DIR -o val.json
    python tools/validate_lm.py --synthetic [--synthetic_items 4] [--synthetic_tokens 64] -o val.json

VALID_DIR is laid out like the reference's validation set (text2semantic/roformer/dataloader.py:124-160): utt/<name>.npy holds the object
array (phones, tones, lang_ids, word2ph) and semantic_token/<name>.npy the item's token ids; BOS and EOS are put around the tokens as the
loader does, labels = tokens, batch size 1.  The speaker id of every item is --spk_id (the reference numbers the speakers in the order
its loader meets their directories).  --synthetic scores seeded items under seeded weights (no checkpoint ships).

The logits behind the numbers are the causal (prefix) ones that `generate` computes, not those of the reference's one-call forward on
transformers 5.x, which sees the future tokens: on real weights the loss is the causal cross-entropy.

--lm_type llama (or a checkpoint whose config.yaml names the Llama): Llama.score over the stream [108, phones, 109, 108 + K, tokens + 108, EOS]
(reference llama.py:98-101).  "loss" and the accuracy are then those of labels = input_ids -- every id of the stream, phones included, over the
full vocabulary: the reference's training loss (text2semantic/llama/dataloader.py:182-183; its forward is causal) -- and
"semantic_loss" / "semantic_top<k>_acc" next to them count the semantic tokens and the EOS only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-m", "--model", help="exp/lm/model_<step>.pt ({'model': Roformer.state_dict()}) with config.yaml next to it")
    ap.add_argument("-d", "--data", help="directory with utt/*.npy and semantic_token/*.npy")
    ap.add_argument("-o", "--out", default=None, help="JSON file for the result (always printed)")
    ap.add_argument("-id", "--spk_id", type=int, default=1)
    ap.add_argument("-k", "--topk", type=int, default=5)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--lm_type", default="roformer", choices=("roformer", "llama"), help="which seeded LM --synthetic builds (a checkpoint's config.yaml names its own)")
    ap.add_argument("--synthetic_items", type=int, default=4)
    ap.add_argument("--synthetic_tokens", type=int, default=64)
    a = ap.parse_args(argv)
    if not a.synthetic and not (a.model and a.data):
        ap.error("--model and --data are needed (or --synthetic)")
    if a.topk < 1 or a.synthetic_items < 1 or a.synthetic_tokens < 1:
        ap.error("--topk, --synthetic_items and --synthetic_tokens must be positive")
    return a


def synthetic_items(n_items, n_tokens):
    """(name, phones [L], tones [L], tokens [n]) with lengths that differ from item to item"""
    for i in range(n_items):
        L, n = 17 + 5 * i, n_tokens + 3 * i
        yield (f"synthetic_{i}", (np.arange(L) * 7 + i) % 107 + 1, (np.arange(L) * 5 + i) % 12, (np.arange(n) * 131 + 977 * i) % 4096)


def load_items(path):
    utt, sem = os.path.join(path, "utt"), os.path.join(path, "semantic_token")
    for f in sorted(os.listdir(utt)):
        if f.endswith(".npy") and os.path.exists(os.path.join(sem, f)):
            phones, tones = np.load(os.path.join(utt, f), allow_pickle=True)[:2]
            yield f[:-4], np.asarray(phones), np.asarray(tones), np.load(os.path.join(sem, f))


@torch.no_grad()
def validate_llama(lm, items, k=5):
    """`validate` for the decoder-only Llama: per item the stream loss / accuracy (labels = input_ids) and the semantic-only ones, both from one
    Llama.score call each; then the means over the items"""
    dev = next(lm.parameters()).device
    key = f"top{k}_acc"
    rows = []
    for name, phones, tones, tokens in items:
        ph, tn = (torch.from_numpy(np.asarray(v).astype(np.int64))[None].to(dev) for v in (phones, tones))
        sem = torch.from_numpy(np.asarray(tokens).astype(np.int64))[None].to(dev)
        mask = torch.ones_like(sem)      # every given token counts, whatever its id
        ids, lens, _, _, _ = lm.score_streams(ph, sem, semantic_attention_mask=mask, append_eos=True)
        full = lm.score_ids(ids)      # labels = input_ids: the reference's training loss
        part = lm.score(ph, tn, sem, semantic_attention_mask=mask, append_eos=True)
        rows.append({"name": name, "tokens": int(full.n_tokens), "loss": float(full.loss), key: float((full.ranks[full.ranks >= 0] < k).float().mean()),
                     "semantic_tokens": int(part.n_tokens), "semantic_loss": float(part.loss),
                     "semantic_" + key: float((part.ranks[part.ranks >= 0] < k).float().mean())})
    if not rows:
        raise SystemExit("no items")
    return dict({"items": rows}, **{f: float(np.mean([r[f] for r in rows])) for f in ("loss", key, "semantic_loss", "semantic_" + key)})


@torch.no_grad()
def validate(lm, items, spk_id=1, k=5):
    """-> {"items": [{"name", "tokens", "loss", "top<k>_acc"}], "loss", "top<k>_acc"}: the means over the items, as the reference's loop forms them"""
    if hasattr(lm, "llama"):
        return validate_llama(lm, items, k)
    dev = next(lm.parameters()).device
    key = f"top{k}_acc"
    rows = []
    for name, phones, tones, tokens in items:
        ph, tn = (torch.from_numpy(np.asarray(v).astype(np.int64))[None].to(dev) for v in (phones, tones))
        sem = np.concatenate([[lm.semantic_bos_token_id], np.asarray(tokens).astype(np.int64), [lm.semantic_eos_token_id]])
        sem = torch.from_numpy(sem)[None].to(dev)
        r = lm.score(ph, tn, sem, labels=sem, spk_id=torch.ones_like(ph) * spk_id)
        rows.append({"name": name, "tokens": int(r.n_tokens), "loss": float(r.loss), key: float((r.ranks[r.ranks >= 0] < k).float().mean())})
    if not rows:
        raise SystemExit("no items")
    return {"items": rows, "loss": float(np.mean([r["loss"] for r in rows])), key: float(np.mean([r[key] for r in rows]))}


def main(argv=None):
    a = parse_args(argv)
    import infer_tts
    if a.synthetic:
        lm = infer_tts.synthetic_llama("cuda") if a.lm_type == "llama" else infer_tts.synthetic_lm("cuda")
        items = synthetic_items(a.synthetic_items, a.synthetic_tokens)
    else:
        lm, items = infer_tts.load_lm(a.model, "cuda"), load_items(a.data)
    res = validate(lm, items, a.spk_id, a.topk)
    print(json.dumps(res, indent=1))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)
    return res


if __name__ == "__main__":
    main()
