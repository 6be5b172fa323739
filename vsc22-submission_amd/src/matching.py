"""Matching-track candidate features: per-pair frame x frame similarity matrices on the HIP path.

Mirrors VSC22-Matching-Track-1st/infer/src/utils.py (same function names -- including the reference's
spellings -- arguments and return structure) for the part of `infer_matching.py` that sits between the
candidate search and the classifier / refinement networks:

  * ``generate_candidates_classfiy_feature``  utils.py:21-51   similarity maps fed to the match classifier
  * ``generate_matching_feature``             utils.py:54-77   (query view, reference) feature pairs for refinement
  * ``calclualte_low_var_dim``                utils.py:7-10
  * ``transform_features``                    utils.py:12-16
  * ``search_candidate_pairs``                infer_matching.py:229-262   candidate (query video, reference video) search
  * ``MatchRefineDataset``                    src/dataset.py:127-144      padded maps fed to the refinement networks
  * ``match_classify`` / ``match_refine``     infer_matching.py:158-204   the MobileNetV3 pair classifier and the HRNet
                                              refinement net (vsc_hip/cnn.py: fp32 convolutions on the HIP path)

The reference runs one ``np.matmul(qfeat, rfeat.T)`` per candidate on the host (twice: once to pick the query
view, once for the map).  Here every candidate of a call goes through ONE ``vsc_pair_similarity_f32`` launch
over concatenated frame banks; each score is an independent ascending-k fp32 chain, so the map of the chosen
view is a row slice of the full product -- bit for bit -- and nothing is multiplied twice.

``classify_candidates_hip`` / ``refine_candidates_hip`` (``infer_matching.py --maps hip``) are the same two steps with the
matrices left where the launch wrote them: ``vsc_match_maps_f32`` picks each candidate's query view and writes the cropped,
zero-padded, 3-channel network inputs on the device -- the same bits as ``_best_view`` + the two datasets below -- so neither
a similarity matrix nor a network input crosses PCIe.

``generate_matching_result`` (utils.py:80-116) -- post-processing of the refinement networks' probability maps, cv2
connected components + sklearn RANSAC in the reference -- has two backends.  ``"host"`` (the default) mirrors it as host
code with ``scipy.ndimage.label`` in cv2's place (cv2 is not a dependency here).  ``"hip"`` runs it on the device
(``vsc_match_segments_f32``: one workgroup per (map, threshold), all of them in one launch) under the contract stated in
include/vsc_hip.h -- sklearn's loop with the trial phase in exact integer arithmetic -- and needs neither scipy nor
sklearn; with ``match_refine(..., device_maps=True)`` the probability maps never leave the device.
"""
import dataclasses
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

TOP_ROWS = 10  # rows whose maxima are averaged to score a query view (utils.py:41)
SEARCH_THRESHOLD = -0.1  # infer_matching.py:62


def calclualte_low_var_dim(score_norm_refs, device: str = "host") -> int:
    """Index of the descriptor dimension with the smallest variance over all reference frames.  device="hip": the variance on the
    device (vsc_column_var_f32, numpy's bits); `score_norm_refs` may then be a `ScoreNormBank`, which keeps the set uploaded for the
    normalisation that follows."""
    if device != "host":
        from vsc.baseline.score_normalization import low_variance_dim
        return low_variance_dim(score_norm_refs, device=device)
    sn_features = np.concatenate([ref.feature for ref in score_norm_refs], axis=0)
    return int(sn_features.var(axis=0).argmin())


def transform_features(features, transform: Callable[[np.ndarray], np.ndarray]):
    return [dataclasses.replace(feature, feature=transform(feature.feature)) for feature in features]


def _hip_video_pair_max(q_bank, q_video, n_q_videos, r_bank, r_video, n_r_videos, threshold):
    import torch

    from vsc_hip import _lib, ops
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    lims, rv, sc = ops.video_pair_max(torch.from_numpy(q_bank).to(dev), torch.from_numpy(q_video).to(dev), n_q_videos,
                                      torch.from_numpy(r_bank).to(dev), torch.from_numpy(r_video).to(dev), n_r_videos,
                                      threshold)
    return lims.cpu().numpy(), rv.cpu().numpy(), sc.cpu().numpy()


def _bank_with_video_index(videos):
    feats = [np.ascontiguousarray(v.feature, dtype=np.float32) for v in videos]
    dim = feats[0].shape[1] if feats else 0
    bank = np.concatenate(feats, axis=0) if feats else np.zeros((0, dim), np.float32)
    index = np.repeat(np.arange(len(feats), dtype=np.int32), [len(f) for f in feats])
    return bank, index


def search_candidate_pairs(sn_query_list, sn_refs, threshold: float = SEARCH_THRESHOLD,
                           video_pair_max: Optional[Callable] = None) -> List[Tuple[str, str, np.float32]]:
    """Candidate (query_id, ref_id, score) triples, best first (infer_matching.py:229-262).

    The reference searches the flat inner-product index per query video for the top 1024 references of every
    frame, re-runs ``range_search`` for the frames whose 1024th score still exceeds the threshold, and keeps the
    best frame score of every (query video, reference video) in a dict.  Both branches together select exactly
    the frame pairs scoring above ``threshold``, so one ``vsc_video_pair_max_f32`` sweep over all query frames
    and all reference frames yields the dict's contents; what remains here is the sort.  Order: descending
    score; pairs with bit-equal scores follow (query video, reference video) order where the reference keeps
    their first-encounter order -- the only difference, and one that needs an exact fp32 tie across pairs.
    ``video_pair_max(q_bank, q_video, n_q, r_bank, r_video, n_r, threshold) -> (lims, ref_video, score)`` is a
    test seam; the default is the HIP path."""
    if len(sn_query_list) == 0 or len(sn_refs) == 0:
        return []
    q_bank, q_video = _bank_with_video_index(sn_query_list)
    r_bank, r_video = _bank_with_video_index(sn_refs)
    if len(q_bank) == 0 or len(r_bank) == 0:
        return []
    lims, ref_video, score = (video_pair_max or _hip_video_pair_max)(
        q_bank, q_video, len(sn_query_list), r_bank, r_video, len(sn_refs), float(threshold))
    query_video = np.repeat(np.arange(len(sn_query_list)), np.diff(lims))
    order = np.lexsort((ref_video, query_video, -score.astype(np.float64)))
    return [(sn_query_list[query_video[i]].video_id, sn_refs[ref_video[i]].video_id, score[i]) for i in order]


def _hip_pair_similarity(q_bank: np.ndarray, r_bank: np.ndarray, pairs: np.ndarray):
    import torch

    from vsc_hip import _lib, ops
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    flat, offsets = ops.pair_similarity(torch.from_numpy(q_bank).to(dev), torch.from_numpy(r_bank).to(dev), pairs)
    return flat.cpu().numpy(), offsets


class _Banks:
    """Concatenated frame banks of the videos a candidate list touches + the pair table of the launch."""

    def __init__(self, query: Dict[str, np.ndarray], ref: Dict[str, np.ndarray], candidates: Sequence[Tuple]):
        self.q_rows: Dict[str, Tuple[int, int]] = {}
        self.r_rows: Dict[str, Tuple[int, int]] = {}
        q_parts, r_parts = [], []
        nq = nr = 0
        for qid, rid, _ in candidates:
            if qid not in self.q_rows:
                f = np.ascontiguousarray(query[qid], dtype=np.float32)
                self.q_rows[qid] = (nq, len(f))
                q_parts.append(f)
                nq += len(f)
            if rid not in self.r_rows:
                f = np.ascontiguousarray(ref[rid], dtype=np.float32)
                self.r_rows[rid] = (nr, len(f))
                r_parts.append(f)
                nr += len(f)
        dim = q_parts[0].shape[1] if q_parts else 0
        self.q_bank = np.concatenate(q_parts, axis=0) if q_parts else np.zeros((0, dim), np.float32)
        self.r_bank = np.concatenate(r_parts, axis=0) if r_parts else np.zeros((0, dim), np.float32)
        self.pairs = np.array([[*self.q_rows[qid], *self.r_rows[rid]] for qid, rid, _ in candidates],
                              dtype=np.int64).reshape(-1, 4)


def pair_similarity_matrices(query: Dict[str, np.ndarray], ref: Dict[str, np.ndarray], candidates: Sequence[Tuple],
                             pair_similarity: Optional[Callable] = None) -> List[np.ndarray]:
    """[q_frames, r_frames] similarity matrix of every (qid, rid, score) candidate, one launch for all of them.
    ``pair_similarity(q_bank, r_bank, pairs) -> (flat, offsets)`` is a test seam; the default is the HIP path."""
    if len(candidates) == 0:
        return []
    banks = _Banks(query, ref, candidates)
    flat, off = (pair_similarity or _hip_pair_similarity)(banks.q_bank, banks.r_bank, banks.pairs)
    return [flat[off[i]:off[i + 1]].reshape(int(banks.pairs[i, 1]), int(banks.pairs[i, 3]))
            for i in range(len(candidates))]


def _best_view(sim_mat: np.ndarray, num_data: int) -> int:
    """Start row of the query view (block of ``num_data`` rows) whose ten best row maxima have the largest mean
    (utils.py:35-44); the first such view on ties, as np.argmax."""
    best, best_score = 0, None
    for start in range(0, sim_mat.shape[0], num_data):
        maxs = np.sort(sim_mat[start:start + num_data].max(1))
        score = maxs[-TOP_ROWS:].mean()
        if best_score is None or score > best_score:
            best, best_score = start, score
    return best


def generate_candidates_classfiy_feature(query, ref, candidate_list, query_video_len_map, pair_similarity=None):
    """-> (features, infos): per candidate the [q, r] map and, wrapped in a list as in the reference, its [r, q]
    transpose; infos repeats [qid, rid, score] for both."""
    mats = pair_similarity_matrices(query, ref, candidate_list, pair_similarity)
    features, infos = [], []
    for (qid, rid, score), sim_mat in zip(candidate_list, mats):
        num_data = query_video_len_map[qid]
        if num_data != sim_mat.shape[0]:
            start = _best_view(sim_mat, num_data)
            sim_mat = sim_mat[start:start + num_data]
        features.append(np.ascontiguousarray(sim_mat))
        infos.append([qid, rid, score])
        features.append([np.ascontiguousarray(sim_mat.T)])
        infos.append([qid, rid, score])
    return features, infos


def generate_matching_feature(query, ref, query_video_len_map, candidate_score_list, pair_similarity=None):
    """-> [[qid, rid, qfeat (the selected view's rows), rfeat], ...]"""
    mats = pair_similarity_matrices(query, ref, candidate_score_list, pair_similarity)
    res_list = []
    for (qid, rid, _), sim_mat in zip(candidate_score_list, mats):
        num_data = query_video_len_map[qid]
        qfeat = query[qid]
        if num_data != len(qfeat):
            start = _best_view(sim_mat, num_data)
            qfeat = qfeat[start:start + num_data]
        res_list.append([qid, rid, qfeat, ref[rid]])
    return res_list


class MatchClassifyDataset:
    """Similarity maps cropped / zero-padded to ``resolution`` and repeated on 3 channels (src/dataset.py:103-124)."""

    def __init__(self, features, infos, resolution=(160, 160)):
        self.features, self.infos, self.resolution = features, infos, resolution

    def __len__(self):
        return len(self.features)

    def __getitem__(self, item):
        feature = self.features[item]
        if isinstance(feature, list):
            feature = feature[0]
        h, w = min(feature.shape[0], self.resolution[0]), min(feature.shape[1], self.resolution[1])
        canvas = np.zeros(self.resolution, dtype=np.float32)
        canvas[:h, :w] = feature[:h, :w]
        return np.stack([canvas] * 3), self.infos[item][0], self.infos[item][1]


class MatchRefineDataset:
    """(query view, reference) similarity maps cropped / zero-padded to ``resolution``, repeated on 3 channels, with
    the valid height and width (src/dataset.py:127-144).  The reference multiplies ``qfeat @ rfeat.T`` per item on
    the host; here the maps of all items come from one ``vsc_pair_similarity_f32`` launch on first access."""

    def __init__(self, meta, resolution=(160, 160), pair_similarity: Optional[Callable] = None):
        self.meta, self.resolution, self._pair_similarity = meta, resolution, pair_similarity
        self._maps: Optional[List[np.ndarray]] = None

    def __len__(self):
        return len(self.meta)

    def _similarity_maps(self) -> List[np.ndarray]:
        if self._maps is None:
            query = {i: m[2] for i, m in enumerate(self.meta)}
            ref = {i: m[3] for i, m in enumerate(self.meta)}
            self._maps = pair_similarity_matrices(query, ref, [(i, i, 0.0) for i in range(len(self.meta))],
                                                  self._pair_similarity)
        return self._maps

    def __getitem__(self, item):
        qid, rid = self.meta[item][0], self.meta[item][1]
        sim_mat = self._similarity_maps()[item]
        h, w = min(sim_mat.shape[0], self.resolution[0]), min(sim_mat.shape[1], self.resolution[1])
        feat = np.zeros(self.resolution, dtype=np.float32)
        feat[:h, :w] = sim_mat[:h, :w]
        return np.stack([feat, feat, feat]), qid, rid, h, w


# ---- the two networks between candidate search and localisation (infer_matching.py:158-204) -------------------
MATCH_CLS_RESOLUTION, MATCH_REFINE_RESOLUTION = (160, 160), (224, 224)   # infer_matching.py:159,178
MATCH_CLS_BATCH, MATCH_REFINE_BATCH = 2048, 16                           # infer_matching.py:160,179


def load_match_models(cls_state_dicts, refine_state_dicts, device="cuda"):
    """State dicts of the reference's ClassifyModel / HRnet modules (train/models.py; timm parameter names; a
    torch.jit.load(...).state_dict() of the shipped submit_cls_model*.pt / submit_match_model*.pt has them) ->
    (classifier models, refinement models) on the HIP path."""
    from vsc_hip import cnn
    return ([cnn.MobileNetV3SmallHip(sd, device) for sd in cls_state_dicts],
            [cnn.HRNetRefineHip(sd, device) for sd in refine_state_dicts])


def match_classify(cls_models, match_cls_feature, match_cls_info, batch_size: int = MATCH_CLS_BATCH, device="cuda"):
    """Main.match_classify (infer_matching.py:158-175): probability of "this candidate pair holds a copy" per candidate,
    averaged over the classifier models.  -> list of (query_id, ref_id, prob) in candidate order (the reference builds a
    DataFrame with these three columns)."""
    import torch

    from vsc_hip import cnn
    data = MatchClassifyDataset(match_cls_feature, match_cls_info, MATCH_CLS_RESOLUTION)
    out = []
    for lo in range(0, len(data), batch_size):
        items = [data[i] for i in range(lo, min(lo + batch_size, len(data)))]
        feature = torch.from_numpy(np.stack([it[0] for it in items])).to(device)
        prob = cnn.match_classify_probability(cls_models, feature).cpu().numpy()
        out.extend((it[1], it[2], float(p)) for it, p in zip(items, prob))
    return out


@dataclasses.dataclass
class DeviceProbabilityMaps:
    """The cropped probability maps of match_refine(..., device_maps=True): map i is the row-major [h, w] block of `flat`
    (a float32 device tensor) at element offset items[i, 0], with items[i] = (offset, h, w) and ids[i] = (qid, rid)."""
    ids: List[Tuple[str, str]]
    items: np.ndarray
    flat: object

    def __len__(self):
        return len(self.ids)


def match_refine(refine_models, match_meta, batch_size: int = MATCH_REFINE_BATCH, device="cuda", pair_similarity=None,
                 device_maps: bool = False):
    """Main.match_refine (infer_matching.py:177-204): per candidate the copy-probability map over (query frame, ref frame),
    averaged over the refinement models and over each model's transposed pass, cropped to the valid h x w.
    -> [[qid, rid, probability map [h, w], similarity map [h, w]], ...], the input of generate_matching_result; with
    ``device_maps=True`` a DeviceProbabilityMaps instead: the cropped maps stay on the device as one flat buffer plus a
    table (the input of generate_matching_result(..., backend="hip"))."""
    import torch

    from vsc_hip import cnn
    data = MatchRefineDataset(match_meta, MATCH_REFINE_RESOLUTION, pair_similarity)
    res_list, ids, table, parts, offset = [], [], [], [], 0
    for lo in range(0, len(data), batch_size):
        items = [data[i] for i in range(lo, min(lo + batch_size, len(data)))]
        feature = torch.from_numpy(np.stack([it[0] for it in items]))
        pred = cnn.match_refine_probability(refine_models, feature.to(device))
        if device_maps:
            for i, (_, qid, rid, h, w) in enumerate(items):
                parts.append(pred[i, 1, :h, :w].reshape(-1))
                ids.append((qid, rid))
                table.append((offset, h, w))
                offset += h * w
            continue
        pred = pred.cpu().numpy()
        for i, (fea, qid, rid, h, w) in enumerate(items):
            res_list.append([qid, rid, pred[i][1][:h, :w], fea[0][:h, :w]])
    if device_maps:
        flat = torch.cat(parts) if parts else torch.empty(0, dtype=torch.float32, device=device)
        return DeviceProbabilityMaps(ids, np.array(table, dtype=np.int64).reshape(-1, 3), flat)
    return res_list


# ---- steps 3 and 4 with the maps kept on the device (infer_matching.py --maps hip) ------------------------------
MATCH_MAPS_FLOAT_BUDGET = 1 << 28   # similarities (fp32 values) of one vsc_pair_similarity_f32 + vsc_match_maps_f32 call: 1 GiB
MATCH_REFINE_GROUP = 64             # refinement batches whose canvases are built by one call (224 x 224 x 3 floats per candidate)


def _map_shape(query, ref, candidate, len_map, resolution: int):
    """(similarity rows, columns, frames per view) the canvas of one candidate needs.  A multi-view candidate needs every row
    and every column (the view is chosen over all of them); a single-view one only the corner the canvas shows -- any slice of a
    larger product is the same bits (vsc_pair_similarity_f32)."""
    qid, rid = candidate[0], candidate[1]
    q_rows, r_rows, frames = len(query[qid]), len(ref[rid]), int(len_map[qid])
    if frames < 1:
        raise ValueError(f"{qid}: {frames} frames per view")
    if q_rows > frames:
        if q_rows % frames:
            raise ValueError(f"{qid}: {q_rows} descriptors are not whole views of {frames} frames -- the device path needs whole "
                             "views (vsc_match_maps_f32); run with --maps host")
        return q_rows, r_rows, frames
    return min(q_rows, resolution), min(r_rows, resolution), frames


def _device_canvases(query, ref, candidates, len_map, resolution: int, with_transpose: bool):
    """Network inputs of a candidate list, built on the device: -> (float32 device tensor [n * (1 + with_transpose), 3, R, R],
    channels last in memory -- the chosen view's map of every candidate and, with the transpose, its transposed map right behind
    it --, [(valid height, valid width)] per candidate).  _Banks -> vsc_pair_similarity_f32 -> vsc_match_maps_f32, in as many
    calls as MATCH_MAPS_FLOAT_BUDGET asks for; nothing is copied back and nothing waits for the device."""
    shapes = [_map_shape(query, ref, c, len_map, resolution) for c in candidates]   # raises for ragged views: before any device work
    import torch

    from vsc_hip import _lib, ops
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, slices = len(candidates), 2 if with_transpose else 1
    out = torch.empty((n * slices, resolution, resolution, 3), dtype=torch.float32, device=dev)   # every element is written
    lo = 0
    while lo < n:
        hi, floats = lo, 0
        while hi < n and (hi == lo or floats + shapes[hi][0] * shapes[hi][1] <= MATCH_MAPS_FLOAT_BUDGET):
            floats += shapes[hi][0] * shapes[hi][1]
            hi += 1
        banks = _Banks(query, ref, candidates[lo:hi])
        pairs = banks.pairs.copy()
        pairs[:, 1] = [s[0] for s in shapes[lo:hi]]
        pairs[:, 3] = [s[1] for s in shapes[lo:hi]]
        items = np.zeros((hi - lo, 4), dtype=np.int64)
        if floats:
            flat, off = ops.pair_similarity(torch.from_numpy(banks.q_bank).to(dev), torch.from_numpy(banks.r_bank).to(dev), pairs)
            items[:, 0] = off[:-1]
        else:                                  # only empty matrices: all-zero canvases
            flat = torch.empty(0, dtype=torch.float32, device=dev)
        items[:, 1], items[:, 2], items[:, 3] = pairs[:, 1], pairs[:, 3], [s[2] for s in shapes[lo:hi]]
        ops.match_maps(flat, items, resolution, with_transpose, out=out[lo * slices:hi * slices])
        lo = hi
    hw = [(min(f, q, resolution), min(r, resolution)) for q, r, f in shapes]
    return out.permute(0, 3, 1, 2), hw


def classify_candidates_hip(cls_models, query, ref, candidate_list, len_map, batch_size: int = MATCH_CLS_BATCH):
    """generate_candidates_classfiy_feature + match_classify without a similarity matrix or a network input crossing PCIe:
    -> the same [(query_id, ref_id, prob), ...], two rows per candidate (its map, then the transposed map).  Works in groups of
    batch_size // 2 candidates, so every network batch holds exactly the items of the host path's batch; only the
    probabilities are copied back.  Raises ValueError for a query whose rows are not whole views (ragged --query_frames)."""
    from vsc_hip import cnn
    assert batch_size >= 2 and batch_size % 2 == 0, "a candidate's map and its transpose share a batch"
    candidate_list = list(candidate_list)
    out = []
    for lo in range(0, len(candidate_list), batch_size // 2):
        group = candidate_list[lo:lo + batch_size // 2]
        feature, _ = _device_canvases(query, ref, group, len_map, MATCH_CLS_RESOLUTION[0], True)
        prob = cnn.match_classify_probability(cls_models, feature).cpu().numpy()
        for i, (qid, rid, _) in enumerate(group):
            out.append((qid, rid, float(prob[2 * i])))
            out.append((qid, rid, float(prob[2 * i + 1])))
    return out


def refine_candidates_hip(refine_models, query, ref, len_map, candidate_score_list, device_maps: bool = False,
                          batch_size: int = MATCH_REFINE_BATCH):
    """generate_matching_feature + match_refine with the (query view, reference) maps chosen, cropped and padded on the device:
    -> match_refine's rows [[qid, rid, probability map [h, w], similarity map [h, w]], ...] (the similarity map is the canvas's
    crop, copied back), or with ``device_maps=True`` its DeviceProbabilityMaps -- then only the table is host data.  The network
    batches are those of match_refine."""
    import torch

    from vsc_hip import cnn
    candidate_score_list = list(candidate_score_list)
    res_list, ids, table, parts, offset = [], [], [], [], 0
    group = batch_size * MATCH_REFINE_GROUP
    for glo in range(0, len(candidate_score_list), group):
        cands = candidate_score_list[glo:glo + group]
        canvas, hw = _device_canvases(query, ref, cands, len_map, MATCH_REFINE_RESOLUTION[0], False)
        for lo in range(0, len(cands), batch_size):
            feature = canvas[lo:lo + batch_size]
            pred = cnn.match_refine_probability(refine_models, feature)
            if device_maps:
                for i, ((qid, rid, _), (h, w)) in enumerate(zip(cands[lo:lo + batch_size], hw[lo:])):
                    parts.append(pred[i, 1, :h, :w].reshape(-1))
                    ids.append((qid, rid))
                    table.append((offset, h, w))
                    offset += h * w
                continue
            pred, sims = pred.cpu().numpy(), feature[:, 0].contiguous().cpu().numpy()
            for i, ((qid, rid, _), (h, w)) in enumerate(zip(cands[lo:lo + batch_size], hw[lo:])):
                res_list.append([qid, rid, pred[i][1][:h, :w], sims[i][:h, :w]])
    if device_maps:
        flat = torch.cat(parts) if parts else torch.empty(0, dtype=torch.float32, device="cuda")
        return DeviceProbabilityMaps(ids, np.array(table, dtype=np.int64).reshape(-1, 3), flat)
    return res_list


# ---- localisation from the refinement maps (host code, utils.py:80-116) ---------------------------------------
MIN_COMPONENT = 10      # a connected component needs more pixels than this to be fitted on its own
RANSAC_TRIALS, RANSAC_SEED, RANSAC_RESIDUAL = 200, 2023, 2


def _components8(mask: np.ndarray):
    """8-connected components of a boolean map -> (labels, count); 0 = background, components numbered in raster
    order of their first pixel (cv2 may number them differently; nothing downstream depends on the numbering)."""
    from scipy import ndimage
    labels, count = ndimage.label(mask, structure=np.ones((3, 3), dtype=np.int32))
    return labels.astype(np.int32), int(count)


def _fit_segment(prob_map: np.ndarray, x: np.ndarray, y: np.ndarray, std_ratio: float):
    """Weighted RANSAC line y = f(x) through the pixels (x = query frame, y = reference frame) -> the matched
    segment [q_start, r_start, q_end, r_end, score] or None."""
    from sklearn.linear_model import RANSACRegressor
    if len(set(x)) <= 3:
        return None
    ransac = RANSACRegressor(max_trials=RANSAC_TRIALS, random_state=RANSAC_SEED, residual_threshold=RANSAC_RESIDUAL)
    ransac.fit(x[:, np.newaxis], y[:, np.newaxis], sample_weight=np.square(prob_map[x, y]))
    on_line = abs(y - ransac.predict(x[:, np.newaxis]).flatten()) < 1
    slope = ransac.estimator_.coef_[0][0]
    if slope <= 0:
        return None
    slope = max(1 / slope, slope)
    xs, ys = x[on_line], y[on_line]
    if not (on_line.sum() > 5 and len(set(xs)) > 3 and len(set(ys)) > 3):
        return None
    top = prob_map[xs, ys]
    return [xs[0], ys[0], xs[-1], ys[-1], top.max() - top.std() * std_ratio - abs(slope - 1) / 10]


def _to_device_maps(res_list) -> DeviceProbabilityMaps:
    """Host rows [[qid, rid, probability map, _], ...] (or a DeviceProbabilityMaps, returned as it is) -> device maps."""
    import torch
    if isinstance(res_list, DeviceProbabilityMaps):
        return res_list
    ids, table, parts, offset = [], [], [], 0
    for qid, rid, prob_map, _ in res_list:
        prob_map = np.ascontiguousarray(prob_map, dtype=np.float32)
        h, w = prob_map.shape
        ids.append((qid, rid))
        table.append((offset, h, w))
        parts.append(prob_map.reshape(-1))
        offset += h * w
    flat = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    dev = torch.device("cuda", torch.cuda.current_device())
    return DeviceProbabilityMaps(ids, np.array(table, dtype=np.int64).reshape(-1, 3), torch.from_numpy(flat).to(dev))


def generate_matching_results_hip(res_list, passes, max_segments: int = 8):
    """The device backend of generate_matching_result for several (threshold, std_ratio) passes at once: one
    vsc_match_segments_f32 launch over every (map, pass), one copy back of the segments.  -> one row list per pass, rows
    [qid, rid, q_start, r_start, q_end, r_end, score] in map order.  Contract: vsc_match_segments_f32 in include/vsc_hip.h."""
    from vsc_hip import _lib, ops
    _lib.require_device()
    passes = [(float(t), float(r)) for t, r in passes]
    out = [[] for _ in passes]
    maps = _to_device_maps(res_list)
    if len(maps) == 0 or not passes:
        return out
    segments, scores, counts = ops.match_segments(maps.flat, maps.items, [t for t, _ in passes], [r for _, r in passes],
                                                  max_segments)
    segments, scores, counts = segments.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()
    for i, (qid, rid) in enumerate(maps.ids):
        for t in range(len(passes)):
            for k in range(int(counts[i, t])):
                out[t].append([qid, rid, *(int(v) for v in segments[i, t, k]), float(scores[i, t, k])])
    return out


def generate_matching_result(res_list, threshold=0.05, std_ratio=2, backend="host"):
    """[[qid, rid, probability map, similarity map], ...] -> [[qid, rid, q_start, r_start, q_end, r_end, score], ...].

    ``backend="hip"`` runs on the device under the contract of vsc_match_segments_f32 (res_list may then also be the
    DeviceProbabilityMaps of match_refine(..., device_maps=True)); it raises HipPathUnavailable without a device.

    Per map: pixels above ``threshold`` are split into 8-connected components; each component of more than ten
    pixels is fitted together with ALL pixels of the small components (or, when there is no large component, the
    small ones are fitted as one set); a fit yields a segment when its slope is positive and enough distinct
    frames lie within one frame of the line.  Same sklearn estimator, seed and thresholds as the reference."""
    if backend == "hip":
        return generate_matching_results_hip(res_list, [(threshold, std_ratio)])[0]
    if backend != "host":
        raise ValueError(f"backend must be 'host' or 'hip', not {backend!r}")
    match_res = []
    for qid, rid, prob_map, _ in res_list:
        loose = prob_map > threshold                 # ends up holding the pixels of the small components only
        labels, count = _components8(loose)
        large = []
        for i in range(1, count + 1):
            member = labels == i
            if member.sum() > MIN_COMPONENT:
                large.append(member)
                loose = loose & ~member
        groups = [member | loose for member in large] if large else [loose]
        for group in groups:
            x, y = np.where(group)
            seg = _fit_segment(prob_map, x, y, std_ratio)
            if seg is not None:
                match_res.append([qid, rid, *seg])
    return match_res
