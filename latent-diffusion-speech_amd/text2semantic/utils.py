"""`get_language_model` with the reference's name and argument convention (reference text2semantic/utils.py:20-28)."""


def get_language_model(**args):
    model_type = args["text2semantic"]["model"]["type"]
    if model_type == "roformer":
        from text2semantic.roformer.roformer import get_model
    elif model_type == "llama":      # (the reference's utils.py has no such branch: its Llama is only ever built by hand, llama.py:186-193)
        from text2semantic.llama.llama import get_model
    else:
        raise ValueError(f" [x] Unknown Model: {model_type}")
    return get_model(args["common"]["n_spk"], **args["text2semantic"])


def get_topk_acc(gt_token, logits, k=5):
    """fraction of positions whose ground-truth token is among the k largest logits (reference text2semantic/utils.py get_topk_acc):
    gt_token [N] int, logits [N, V]"""
    import torch
    topk = torch.topk(logits, k, dim=-1).indices
    return float((topk == gt_token.to(topk.device)[:, None]).any(-1).float().mean())
