"""CSLS-style score normalisation of descriptors against a noise bank
(reference: infer/vsc/baseline/score_normalization.py:34-192).

    sim_sn(q, r) = <q, r> - beta * mean_k top-k <q, noise>

encoded as one extra dimension: query' = [q, bias(q)], ref' = [r, 1].  The nearest-noise
search (`index.search(query.feature, k)`, :95/:141) and the L2 normalisation (:84-88) run
on the GPU through libvsc_hip.so; the bookkeeping stays numpy, as in the reference.

``device="hip"`` on `score_normalize`, `query_score_normalize`, `ref_score_normalize` and `low_variance_dim` is the whole step on the
device: one upload per set, the low-variance dimension from vsc_column_var_f32, the narrowed and normalised rows, the
nearest-noise scores and the bias without leaving it (vsc_score_norm_rows_f32, ops.knn_ip, vsc_score_norm_bias_f32), one download
per result -- the same bytes as the default path.  It takes float32 descriptors, which is what `load_features`
hands out, and raises `HipPathUnavailable` without a device.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, List, Tuple

import numpy as np

from vsc.index import FlatIPBank, VideoFeature


def transform_features(features: List[VideoFeature], transform: Callable) -> List[VideoFeature]:
    return [dataclasses.replace(f, feature=transform(f.feature)) for f in features]


def normalize(x: np.ndarray) -> np.ndarray:
    """sklearn.preprocessing.normalize (l2, axis=1) on the GPU."""
    import torch
    from vsc_hip import ops
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return ops.l2_normalize_(t).cpu().numpy()


def normalize_videos(features: List[VideoFeature], block_rows: int = 1 << 20) -> List[VideoFeature]:
    """`transform_features(features, normalize)` (:84-88) with the videos of a block normalised in ONE device round trip instead of one per
    video (40 k reference videos: 40 k round trips): the kernel is row-wise, the rows are the same bits."""
    out, lo = [], 0
    lens = [len(f) for f in features]
    while lo < len(features):
        hi, rows = lo, 0
        while hi < len(features) and (hi == lo or rows + lens[hi] <= block_rows):
            rows += lens[hi]
            hi += 1
        block = features[lo:hi]
        if rows:
            flat = normalize(np.concatenate([f.feature for f in block]))
            parts = np.split(flat, np.cumsum(lens[lo:hi])[:-1])
        else:
            parts = [f.feature for f in block]
        out.extend(dataclasses.replace(f, feature=p) for f, p in zip(block, parts))
        lo = hi
    return out


DEVICES = ("host", "hip")


def _check_device(device: str, *sets) -> bool:
    """-> True for the device path.  A ScoreNormBank is device memory: it only goes with device="hip"."""
    if device not in DEVICES:
        raise ValueError(f"device {device!r}: one of {DEVICES}")
    if device == "host" and any(isinstance(x, ScoreNormBank) for x in sets):
        raise ValueError("a ScoreNormBank holds its rows on the device: pass device='hip', or the list of VideoFeature")
    return device == "hip"


def host_rows(features: List[VideoFeature]) -> np.ndarray:
    """All rows of the videos as ONE C-contiguous float32 [n, d] array: the base array itself, without a copy, when the videos'
    `feature` arrays are consecutive views of it (what `load_features` hands out); one np.concatenate otherwise."""
    feats = [f.feature for f in features]
    first = feats[0] if feats else None
    base = getattr(first, "base", None)
    if (isinstance(base, np.ndarray) and base.ndim == 2 and base.dtype == np.float32 and base.flags.c_contiguous
            and all(f.base is base and f.ndim == 2 and f.dtype == np.float32 and f.flags.c_contiguous and f.shape[1] == base.shape[1]
                    for f in feats)):
        row_bytes = base.shape[1] * 4
        at = lambda a: a.__array_interface__["data"][0]
        lo, rem = divmod(at(first) - at(base), row_bytes)
        expect, n = at(first), 0
        for f in feats:
            if f.shape[0] and at(f) != expect:
                break
            expect += f.shape[0] * row_bytes
            n += f.shape[0]
        else:
            if rem == 0 and 0 <= lo and lo + n <= base.shape[0]:
                return base[lo:lo + n]
    if not feats:
        raise ValueError("score normalisation of an empty list of videos")
    return np.ascontiguousarray(np.concatenate(feats), dtype=np.float32)


class DeviceRows(list):
    """The list of VideoFeature a device score normalisation returns: the features are row views of one host array, and `rows_dev`
    is that array on the device ([n, d] float32), for a consumer that would otherwise upload it again (VideoIndex.add)."""
    rows_dev = None


class ScoreNormBank:
    """A set of descriptors uploaded once for device="hip": as the normalisation set (in place of the list, in the three functions
    below, `low_variance_dim` and `src.matching.calclualte_low_var_dim`) it computes and caches the low-variance dimension and
    the narrowed, normalised noise bank; as `refs` of `ref_score_normalize` it saves the second upload of a set that is also
    another set's normalisation set (concat_pca_sn.py)."""

    def __init__(self, features: List[VideoFeature]):
        import torch
        from vsc_hip import _lib
        _lib.require_device()
        self.features = list(features)
        self.video_ids = {f.video_id for f in self.features}
        self.rows = torch.from_numpy(host_rows(self.features)).cuda()      # [n, d]: the one upload of the set
        self._dim = None
        self._noise = {}

    def __len__(self):
        return len(self.features)

    def __iter__(self):
        return iter(self.features)

    def low_variance_dim(self) -> int:
        if self._dim is None:
            from vsc_hip import ops
            self._dim = int(np.argmin(ops.column_var(self.rows).cpu().numpy()))    # argmin on the host: numpy's tie and NaN rules
        return self._dim

    def noise(self, drop: int, l2_normalize: bool):
        """the bank the queries are searched against: the rows without column `drop` (-1: all columns), normalised"""
        if drop < 0 and not l2_normalize:
            return self.rows
        key = (int(drop), bool(l2_normalize))
        if key not in self._noise:
            from vsc_hip import ops
            self._noise[key] = ops.score_norm_rows(self.rows, drop, l2_normalize, 0)
        return self._noise[key]


def _as_bank(x) -> ScoreNormBank:
    return x if isinstance(x, ScoreNormBank) else ScoreNormBank(x)


def _finish(features: List[VideoFeature], rows_dev) -> "DeviceRows":
    """the one device -> host copy of a result; the videos are row views of it (a video without rows: a (0, width) block)"""
    host = rows_dev.cpu().numpy()
    out, lo = DeviceRows(), 0
    for f in features:
        out.append(dataclasses.replace(f, feature=host[lo:lo + len(f)]))
        lo += len(f)
    assert lo == host.shape[0]
    out.rows_dev = rows_dev
    return out


def _device_queries(queries, bank: ScoreNormBank, drop: int, l2_normalize: bool, beta: float, nk: int, gated=None) -> "DeviceRows":
    """[normalize(delete(q, drop)), bias(q)]: rows kernel -> nearest-noise search -> bias kernel -> rows kernel, all on the device.
    gated: per video, True where the bias is -100 (a video below the score threshold)."""
    import torch
    from vsc_hip import ops
    x = torch.from_numpy(host_rows(queries)).cuda()
    narrowed = ops.score_norm_rows(x, drop, l2_normalize, 0)
    sims, _ = ops.knn_ip(narrowed, bank.noise(drop, l2_normalize), nk)
    del narrowed
    gate = None
    if gated is not None:
        gate = torch.from_numpy(np.repeat(np.asarray(gated, dtype=np.uint8), [len(q) for q in queries])).cuda()
    bias = ops.score_norm_bias(sims, nk, beta, gate)
    return _finish(queries, ops.score_norm_rows(x, drop, l2_normalize, 2, last=bias))


def _device_refs(refs, drop: int, l2_normalize: bool) -> "DeviceRows":
    """[normalize(delete(r, drop)), 1]"""
    import torch
    from vsc_hip import ops
    bank = refs if isinstance(refs, ScoreNormBank) else None
    x = bank.rows if bank is not None else torch.from_numpy(host_rows(refs)).cuda()
    return _finish(bank.features if bank is not None else refs, ops.score_norm_rows(x, drop, l2_normalize, 1))


def low_variance_dim(score_norm_refs: List[VideoFeature], device: str = "host") -> int:
    """The dimension given up for the bias term (:74-76; infer/src/utils.py:2-5)."""
    if _check_device(device, score_norm_refs):
        return _as_bank(score_norm_refs).low_variance_dim()
    bank = np.concatenate([r.feature for r in score_norm_refs], axis=0)
    return int(bank.var(axis=0).argmin())


def _noise_bank(score_norm_refs: List[VideoFeature]) -> FlatIPBank:
    bank = FlatIPBank(score_norm_refs[0].dimensions())
    for r in score_norm_refs:
        bank.add(r.feature)
    return bank


def _bias_terms(queries, bank: FlatIPBank, beta: float, nk: int):
    """One batched search for all query videos (the reference loops per video; frames are
    independent so batching changes nothing)."""
    lens = [len(q) for q in queries]
    sims, _ = bank.search(np.concatenate([q.feature for q in queries]), nk)
    bias = -beta * sims[:, :nk].mean(axis=1, keepdims=True)
    return np.split(bias, np.cumsum(lens)[:-1])


def _check_disjoint(refs, score_norm_refs):
    ids = lambda x: x.video_ids if isinstance(x, ScoreNormBank) else {f.video_id for f in x}
    if ids(refs) & ids(score_norm_refs):
        raise Exception("Normalizing on the dataset we're evaluating on is against VSC rules. "
                        "An independent dataset is needed.")


def score_normalize(queries, refs, score_norm_refs, l2_normalize: bool = True, replace_dim: bool = True,
                    beta: float = 1.0, nk: int = 1, device: str = "host") -> Tuple[List[VideoFeature], List[VideoFeature]]:
    hip = _check_device(device, refs, score_norm_refs)
    _check_disjoint(refs, score_norm_refs)
    if hip:
        bank = _as_bank(score_norm_refs)
        drop = bank.low_variance_dim() if replace_dim else -1
        return _device_queries(queries, bank, drop, l2_normalize, beta, nk), _device_refs(refs, drop, l2_normalize)
    if score_norm_refs is not None and replace_dim:
        dim = low_variance_dim(score_norm_refs)
        queries, refs, score_norm_refs = [
            transform_features(x, lambda f: np.delete(f, dim, axis=1)) for x in (queries, refs, score_norm_refs)]
    if l2_normalize:
        queries, refs, score_norm_refs = [normalize_videos(x) for x in (queries, refs, score_norm_refs)]
    bias = _bias_terms(queries, _noise_bank(score_norm_refs), beta, nk)
    adapted_q = [dataclasses.replace(q, feature=np.concatenate([q.feature, b], axis=1)) for q, b in zip(queries, bias)]
    adapted_r = [dataclasses.replace(r, feature=np.concatenate([r.feature, np.ones_like(r.feature[:, :1])], axis=1))
                 for r in refs]
    return adapted_q, adapted_r


def query_score_normalize(queries, score_norm_refs, video_scores: dict, score_threshold: float = 0.001,
                          low_var_dim: int = 0, l2_normalize: bool = True, replace_dim: bool = True,
                          beta: float = 1.0, nk: int = 1, device: str = "host") -> List[VideoFeature]:
    if _check_device(device, score_norm_refs):
        gated = [video_scores[q.metadata().video_id] < score_threshold for q in queries]   # :143
        return _device_queries(queries, _as_bank(score_norm_refs), low_var_dim if replace_dim else -1, l2_normalize, beta, nk, gated)
    if score_norm_refs is not None and replace_dim:
        queries, score_norm_refs = [
            transform_features(x, lambda f: np.delete(f, low_var_dim, axis=1)) for x in (queries, score_norm_refs)]
    if l2_normalize:
        queries, score_norm_refs = [normalize_videos(x) for x in (queries, score_norm_refs)]
    bias = _bias_terms(queries, _noise_bank(score_norm_refs), beta, nk)
    out = []
    for q, b in zip(queries, bias):
        if video_scores[q.metadata().video_id] < score_threshold:
            b = -100.0 * np.ones_like(b)  # :143: videos judged "no copy" are pushed out of every ranking
        out.append(dataclasses.replace(q, feature=np.concatenate([q.feature, b], axis=1)))
    return out


def ref_score_normalize(refs, score_norm_refs, l2_normalize: bool = True, replace_dim: bool = True,
                        beta: float = 1.0, nk: int = 1, device: str = "host") -> List[VideoFeature]:
    hip = _check_device(device, refs, score_norm_refs)
    _check_disjoint(refs, score_norm_refs)
    if hip:
        return _device_refs(refs, _as_bank(score_norm_refs).low_variance_dim() if replace_dim else -1, l2_normalize)
    if score_norm_refs is not None and replace_dim:
        dim = low_variance_dim(score_norm_refs)
        refs = transform_features(refs, lambda f: np.delete(f, dim, axis=1))
    if l2_normalize:
        refs = normalize_videos(refs)
    return [dataclasses.replace(r, feature=np.concatenate([r.feature, np.ones_like(r.feature[:, :1])], axis=1))
            for r in refs]
