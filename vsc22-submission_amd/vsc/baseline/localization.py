"""Candidate pair -> copied segments (interface of the reference's infer/vsc/baseline/localization.py).

Class names, constructor arguments and the `localize` / `localize_all` / `score` hooks are the reference's, so
`sscd_baseline.localize_and_verify` reads the same.  Two things differ underneath:

  * similarity matrices: the reference multiplies `np.matmul(a, b.T)` per candidate on the host (:33-36); here the
    candidates of a `localize_all` call are laid out as one pair table over concatenated frame banks and computed by ONE
    `vsc_pair_similarity_f32` launch (`src.matching.pair_similarity_matrices`);
  * the temporal alignment model of the `VCSL*` classes is the reference's own VCSL code (`vcsl.vta.build_vta_model`, CPU
    graph search), imported late exactly as the reference does (:44) -- or any object with `forward_sim` passed as
    `model=`, such as `vsc_hip.alignment.TnAlignment`.  The `HipTN*` classes need no VCSL: similarity, TN alignment and
    MaxSim stay on the device (one pair-similarity launch and one `vsc_tn_align_f32` launch per `localize_all` call), and
    only boxes and scores come back; they return what `VCSL*(..., model=TnAlignment(...))` returns.  The `HipVCSL*` classes
    are the same with `VCSLLocalization`'s `model_type` argument: TN, DP or HV on the device (`vsc_hip.alignment.build_alignment`).
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from vsc.index import VideoFeature
from vsc.metrics import CandidatePair, Match

Box = Tuple[int, int, int, int]   # (query frame from, ref frame from, query frame to, ref frame to)


def _load_vcsl_model(model_type: str, options: Dict):
    try:
        from vcsl.vta import build_vta_model
    except ImportError as exc:
        raise ImportError("VCSL (the reference's infer/vcsl package) is needed for temporal alignment; put it on "
                          "PYTHONPATH or pass model= with a forward_sim method") from exc
    return build_vta_model(model_type, **options)


class Localization:
    """Turns candidates into matches; subclasses provide `localize` (one candidate) or override `localize_all`."""

    def localize(self, candidate: CandidatePair) -> List[Match]:
        raise NotImplementedError

    def localize_all(self, candidates: Iterable[CandidatePair]) -> List[Match]:
        found: List[Match] = []
        for candidate in candidates:
            found += self.localize(candidate)
        return found


class LocalizationWithMetadata(Localization):
    """Keeps the videos' features and timestamps by id and serves similarity matrices from the HIP path."""

    def __init__(self, queries: Sequence[VideoFeature], refs: Sequence[VideoFeature],
                 pair_similarity: Optional[Callable] = None):
        self.queries = {video.video_id: video for video in queries}
        self.refs = {video.video_id: video for video in refs}
        self._pair_similarity = pair_similarity   # test seam of src.matching.pair_similarity_matrices

    def similarity_all(self, candidates: Sequence[CandidatePair]) -> List[np.ndarray]:
        """One [query frames, ref frames] matrix per candidate, all from a single launch."""
        from src.matching import pair_similarity_matrices
        q_feats = {c.query_id: self.queries[c.query_id].feature for c in candidates}
        r_feats = {c.ref_id: self.refs[c.ref_id].feature for c in candidates}
        table = [(c.query_id, c.ref_id, c.score) for c in candidates]
        return pair_similarity_matrices(q_feats, r_feats, table, self._pair_similarity)

    def similarity(self, candidate: CandidatePair) -> np.ndarray:
        return self.similarity_all([candidate])[0]


class VCSLLocalization(LocalizationWithMetadata):
    """Alignment by a VCSL model over (biased) similarity matrices; every box it returns becomes a `Match` whose
    times are the timestamps of the box's corner frames and whose score comes from the `score` hook."""

    def __init__(self, queries, refs, model_type, similarity_bias=0.0, model=None, pair_similarity=None, **kwargs):
        super().__init__(queries, refs, pair_similarity)
        self.model = model if model is not None else _load_vcsl_model(model_type, kwargs)
        self.similarity_bias = similarity_bias   # some alignment methods do not take negative similarities well

    def similarity_all(self, candidates):
        return [matrix + self.similarity_bias for matrix in super().similarity_all(candidates)]

    def _match(self, candidate: CandidatePair, box: Box, matrix: np.ndarray) -> Match:
        q_from, r_from, q_to, r_to = box
        query, ref = self.queries[candidate.query_id], self.refs[candidate.ref_id]
        segment = Match(candidate.query_id, candidate.ref_id, 0.0,
                        query_start=query.get_timestamps(q_from)[0], query_end=query.get_timestamps(q_to)[1],
                        ref_start=ref.get_timestamps(r_from)[0], ref_end=ref.get_timestamps(r_to)[1])
        return segment._replace(score=self.score(candidate, segment, box, matrix))

    def localize_all(self, candidates: Sequence[CandidatePair]) -> List[Match]:
        candidates = list(candidates)
        if not candidates:
            return []
        keyed = [(f"{c.query_id}-{c.ref_id}", m) for c, m in zip(candidates, self.similarity_all(candidates))]
        aligned = self.model.forward_sim(keyed)
        if len(aligned) != len(candidates):
            raise AssertionError(f"alignment model returned {len(aligned)} results for {len(candidates)} candidates")
        found: List[Match] = []
        for candidate, (key, matrix), (result_key, boxes) in zip(candidates, keyed, aligned):
            if result_key != key:
                raise AssertionError(f"alignment result {result_key!r} does not belong to candidate {key!r}")
            found += [self._match(candidate, tuple(box), matrix) for box in boxes]
        return found

    def localize(self, candidate: CandidatePair) -> List[Match]:
        return self.localize_all([candidate])

    def score(self, candidate: CandidatePair, match: Match, box: Box, similarity: np.ndarray) -> float:
        return 1.0


class VCSLLocalizationMaxSim(VCSLLocalization):
    """Score = best (unbiased) similarity inside the box, with the reference's half-open slicing."""

    def score(self, candidate, match, box, similarity) -> float:
        q_from, r_from, q_to, r_to = box
        return similarity[q_from:q_to, r_from:r_to].max() - self.similarity_bias


class VCSLLocalizationCandidateScore(VCSLLocalization):
    """Score = the candidate's own (descriptor-track) score."""

    def score(self, candidate, match, box, similarity) -> float:
        return candidate.score


class HipTNLocalization(LocalizationWithMetadata):
    """TN alignment on the device: per `localize_all` call one `vsc_pair_similarity_f32` launch over the candidates'
    frame banks, one `vsc_tn_align_f32` launch over the resulting matrices (biased on the fly), then boxes (and MaxSim)
    are copied back and become `Match` rows exactly as `VCSLLocalization._match` builds them."""

    def __init__(self, queries, refs, similarity_bias=0.0, tn_max_step=10, tn_top_k=5, max_path=10, min_sim=0.2,
                 min_length=5, max_iou=0.3):
        from vsc_hip.alignment import TnAlignment
        super().__init__(queries, refs)
        self.model = TnAlignment(tn_max_step=tn_max_step, tn_top_k=tn_top_k, max_path=max_path, min_sim=min_sim,
                                 min_length=min_length, max_iou=max_iou)
        self.similarity_bias = similarity_bias

    def _align(self, candidates: Sequence[CandidatePair]):
        import torch

        from src.matching import _Banks
        from vsc_hip import _lib, ops
        _lib.require_device()
        dev = torch.device("cuda", torch.cuda.current_device())
        banks = _Banks({c.query_id: self.queries[c.query_id].feature for c in candidates},
                       {c.ref_id: self.refs[c.ref_id].feature for c in candidates},
                       [(c.query_id, c.ref_id, c.score) for c in candidates])
        if len(banks.q_bank) == 0 or len(banks.r_bank) == 0:
            flat, offsets = torch.empty(0, dtype=torch.float32, device=dev), np.zeros(len(candidates) + 1, np.int64)
        else:
            flat, offsets = ops.pair_similarity(torch.from_numpy(banks.q_bank).to(dev),
                                                torch.from_numpy(banks.r_bank).to(dev), banks.pairs)
        boxes, counts, maxsim = self.model.align_pair_similarity(flat, offsets, banks.pairs, self.similarity_bias)
        return boxes.cpu().numpy(), counts.cpu().numpy(), maxsim.cpu().numpy()

    def _match(self, candidate: CandidatePair, box: Box, maxsim: np.float32) -> Match:
        q_from, r_from, q_to, r_to = box
        query, ref = self.queries[candidate.query_id], self.refs[candidate.ref_id]
        segment = Match(candidate.query_id, candidate.ref_id, 0.0,
                        query_start=query.get_timestamps(q_from)[0], query_end=query.get_timestamps(q_to)[1],
                        ref_start=ref.get_timestamps(r_from)[0], ref_end=ref.get_timestamps(r_to)[1])
        return segment._replace(score=self.score(candidate, maxsim))

    def localize_all(self, candidates: Sequence[CandidatePair]) -> List[Match]:
        candidates = list(candidates)
        if not candidates:
            return []
        boxes, counts, maxsim = self._align(candidates)
        found: List[Match] = []
        for i, candidate in enumerate(candidates):
            found += [self._match(candidate, tuple(int(v) for v in boxes[i, j]), maxsim[i, j]) for j in range(counts[i])]
        return found

    def localize(self, candidate: CandidatePair) -> List[Match]:
        return self.localize_all([candidate])

    def score(self, candidate: CandidatePair, maxsim: np.float32):
        return 1.0


class HipTNLocalizationMaxSim(HipTNLocalization):
    """`VCSLLocalizationMaxSim` on the device: score = best (unbiased) similarity inside the half-open box."""

    def score(self, candidate, maxsim):
        return maxsim


class HipTNLocalizationCandidateScore(HipTNLocalization):
    """`VCSLLocalizationCandidateScore` on the device: score = the candidate's own score."""

    def score(self, candidate, maxsim):
        return candidate.score


class HipVCSLLocalization(HipTNLocalization):
    """`VCSLLocalization(queries, refs, model_type, ...)` on the device for the models `vsc_hip.alignment.build_alignment`
    holds (TN, DP, HV): `HipTNLocalization`'s launches with the model's own alignment kernel.  Returns what
    `VCSLLocalization(..., model=<that model>)` returns."""

    def __init__(self, queries, refs, model_type, similarity_bias=0.0, **kwargs):
        from vsc_hip.alignment import build_alignment
        LocalizationWithMetadata.__init__(self, queries, refs)
        self.model = build_alignment(model_type, **kwargs)
        self.similarity_bias = similarity_bias

    def _align(self, candidates):
        boxes, counts, maxsim = super()._align(candidates)
        if hasattr(self.model, "max_boxes"):       # DP: the boxes found may outnumber the slots
            from vsc_hip.alignment import check_counts
            check_counts(counts, self.model.max_boxes, [f"{c.query_id}-{c.ref_id}" for c in candidates])
        return boxes, counts, maxsim


class HipVCSLLocalizationMaxSim(HipVCSLLocalization):
    """`VCSLLocalizationMaxSim` on the device.  A box whose half-open extent is empty (HV: a one-cell diagonal) has no
    similarity to take the maximum of: ValueError, as the reference's `.max()` of an empty slice."""

    def localize_all(self, candidates):
        candidates = list(candidates)
        if not candidates:
            return []
        boxes, counts, maxsim = self._align(candidates)
        found: List[Match] = []
        for i, candidate in enumerate(candidates):
            for j in range(counts[i]):
                box = tuple(int(v) for v in boxes[i, j])
                if box[2] <= box[0] or box[3] <= box[1]:
                    raise ValueError(f"pair {candidate.query_id}-{candidate.ref_id}: box {box} has an empty half-open extent, "
                                     f"MaxSim is undefined on it")
                found.append(self._match(candidate, box, maxsim[i, j]))
        return found

    def score(self, candidate, maxsim):
        return maxsim


class HipVCSLLocalizationCandidateScore(HipVCSLLocalization):
    """`VCSLLocalizationCandidateScore` on the device: score = the candidate's own score."""

    def score(self, candidate, maxsim):
        return candidate.score
