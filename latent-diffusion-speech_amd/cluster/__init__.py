"""K-means semantic codebook helpers with the reference's names and behaviour (reference cluster/__init__.py:5-27):
`semantic_codebook.pt` is a torch-saved dict {'n_features_in_', '_n_threads', 'cluster_centers_'} that is poured into a
scikit-learn KMeans object.  The token -> unit-embedding lookup of the TTS path (22_infer_tts.py:43-52,106) is a row gather
of `cluster_centers_`; `codebook_to_device` / lds.native.gather_rows run it in liblds."""
import numpy as np
import torch


def get_cluster_model(ckpt_path):
    from sklearn.cluster import KMeans
    checkpoint = torch.load(ckpt_path, map_location="cpu", weights_only=False)     # numpy arrays inside: not a weights-only file
    km = KMeans(checkpoint["n_features_in_"])
    for key in ("n_features_in_", "_n_threads", "cluster_centers_"):
        km.__dict__[key] = checkpoint[key]
    return km


_codebook = None      # (the centres array, device string, centres on the device, {metric: h}): the last codebook uploaded


def _device_codebook(model, device, metric="l2"):
    """(centres [K, D], h [K]) of a model on `device`.  The last upload is kept and reused only while `model.cluster_centers_` is the very
    same array object: a reassigned codebook is uploaded again, and nothing is stored inside the (picklable) model"""
    global _codebook
    from lds import native
    arr = model.cluster_centers_
    if _codebook is None or _codebook[0] is not arr or _codebook[1] != str(device):
        _codebook = (arr, str(device), codebook_to_device(arr, device), {})
    if metric not in _codebook[3]:
        _codebook[3][metric] = native.kmeans_prepare(_codebook[2], metric)
    return _codebook[2], _codebook[3][metric]


def get_cluster_result(model, x, lengths=None, pad_id=0, metric="l2"):
    """x: np.array [t, dim] -> cluster ids [t] (scikit-learn on the host, as the reference); x a device tensor [t, dim] or [b, t, dim] ->
    int64 ids on the device from liblds (lds_kmeans_assign); with `lengths` ([b] ints) rows at and beyond a clip's length get pad_id.
    metric="cosine" (device path only; a codebook fitted by train_cluster(mode="cosine")): the centre of highest cosine similarity"""
    from lds.native import metric_code
    metric_code(metric)
    if isinstance(x, torch.Tensor):
        from lds import native
        centers, h = _device_codebook(model, x.device, metric)      # (a CPU tensor raises in the binding: there is no CPU fallback)
        x = x.to(torch.float32).contiguous()
        if lengths is not None:
            return native.kmeans_assign(x, centers, h, lengths=lengths, pad_id=pad_id, metric=metric)
        return native.kmeans_assign(x.reshape(-1, x.shape[-1]), centers, h, metric=metric).reshape(x.shape[:-1])
    if lengths is not None:
        raise ValueError("get_cluster_result: lengths= / pad_id= belong to the device path (numpy input is scikit-learn's predict, one clip)")
    if metric != "l2":
        raise ValueError("get_cluster_result: metric= belongs to the device path (numpy input is scikit-learn's Euclidean predict)")
    return model.predict(x)


def get_cluster_center_result(model, x):
    """x: np.array [t, dim] -> the centre of each frame's cluster [t, dim]; a device tensor takes the native path"""
    if isinstance(x, torch.Tensor):
        from lds import native
        return native.gather_rows(_device_codebook(model, x.device)[0], get_cluster_result(model, x))
    return model.cluster_centers_[model.predict(x)]


def train_cluster(features, n_clusters, max_iter=500, tol=1e-2, verbose=False, device="cuda:0", mode="euclidean", **kw):
    """features [n, dim] (numpy or torch) -> the reference's checkpoint dict (17_preprocess_train_cluster.py:43-53, its KMeansGPU branch);
    torch.save it as semantic_codebook.pt and get_cluster_model loads it.  mode: "euclidean" (KMeansGPU, as step 17) or "cosine" (KMeansCosineGPU)"""
    from .kmeans import KMeansCosineGPU, KMeansGPU
    if mode not in ("euclidean", "cosine"):
        raise ValueError(f"train_cluster: mode must be 'euclidean' or 'cosine' (got {mode!r})")
    feats = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)) if isinstance(features, np.ndarray) else features
    if mode == "cosine":
        km = KMeansCosineGPU(n_clusters=n_clusters, verbose=2 if verbose else 0, max_iter=max_iter, tol=tol, device=torch.device(device), **kw)
    else:
        km = KMeansGPU(n_clusters=n_clusters, mode="euclidean", verbose=2 if verbose else 0, max_iter=max_iter, tol=tol, device=torch.device(device), **kw)
    km.fit_predict(feats)
    return {"n_features_in_": int(feats.shape[1]), "_n_threads": 4, "cluster_centers_": km.centroids.cpu().numpy()}


def get_center(model, token):
    return model.cluster_centers_[token]


def codebook_to_device(model_or_centers, device):
    """cluster centres as a contiguous fp32 device tensor [n_codes, dim] for lds.native.gather_rows"""
    centers = getattr(model_or_centers, "cluster_centers_", model_or_centers)
    return torch.from_numpy(np.ascontiguousarray(centers, dtype=np.float32)).to(device)
