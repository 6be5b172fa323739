#!/usr/bin/env python3
"""Descriptor-track evaluation entry point (reference: infer/vsc/baseline/sscd_baseline.py,
run by infer/eval.sh as `python3 -m vsc.baseline.sscd_baseline --query_features ...`).

On the HIP path: optional score normalisation, the exhaustive candidate search
(`search`, sscd_baseline.py:89-103 -> CandidateGeneration.query) and, with ground truth, the
descriptor-track micro-AP (:219-224).  `localize_and_verify` (:107-152) follows: the per-candidate similarity matrices
come from one HIP launch per batch (vsc.baseline.localization).  With `--alignment vcsl` (the default) the temporal
alignment is the reference's own CPU code, and without its VCSL package only candidates.csv is written (in the
reference's format) and matches.csv is skipped with a log line; with `--alignment hip` the alignment and MaxSim run on
the device (vsc_tn_align_f32, or vsc_align_dp_f32 / vsc_align_hv_f32 with `--alignment_model DP` / `HV`) and matches.csv is
written without VCSL.
"""
from __future__ import annotations

import argparse
import logging
import os
from typing import List

from vsc.baseline.score_normalization import score_normalize
from vsc.candidates import CandidateGeneration, MaxScoreAggregation
from vsc.index import VideoFeature
from vsc.metrics import CandidatePair, Dataset, Match, average_precision, micro_average_precision  # noqa: F401
from vsc.storage import load_features, store_features

logger = logging.getLogger("sscd_baseline.py")


def search(queries: List[VideoFeature], refs: List[VideoFeature], retrieve_per_query: float = 1200.0,
           candidates_per_query: float = 25.0, selection: str = "host") -> List[CandidatePair]:
    """selection: "host" (the probe is ordered and grouped on the host) or "hip" (vsc_global_topk_f32 / vsc_pair_first_hits: only
    the candidate pairs leave the device); the same list either way."""
    cg = CandidateGeneration(refs, MaxScoreAggregation(), selection=selection)
    candidates = cg.query(queries, global_k=int(retrieve_per_query * len(queries)), limit=int(candidates_per_query * len(queries)))
    logger.info("Got %d candidates", len(candidates))
    return candidates


ALIGNMENTS = ("vcsl", "hip")
ALIGNMENT_MODELS = ("TN", "DP", "HV")
CANDIDATES = ("host", "hip")
SCORE_NORMS = ("host", "hip")
SEGMENT_METRICS = ("none", "hip")
UAPS = ("host", "hip")


def localize_and_verify(queries: List[VideoFeature], refs: List[VideoFeature], candidates: List[CandidatePair],
                        localize_per_query: float = 5.0, score_normalization: bool = False, model=None,
                        alignment: str = "vcsl", alignment_model: str = "TN") -> List[Match]:
    """sscd_baseline.py:107-152: the best `localize_per_query * len(queries)` candidates, aligned in batches of 512.
    alignment="vcsl": the reference's VCSL model (or `model=`); "hip": the same alignment on the device (vsc_tn_align_f32 /
    vsc_align_dp_f32 / vsc_align_hv_f32), no VCSL needed.  alignment_model: VCSL's model_type, "TN" (the reference's choice),
    "DP" or "HV"; DP and HV get the bias and min_length of the TN call and otherwise their model's defaults."""
    from vsc.baseline.localization import VCSLLocalizationCandidateScore, VCSLLocalizationMaxSim
    if alignment not in ALIGNMENTS:
        raise ValueError(f"alignment {alignment!r}: one of {ALIGNMENTS}")
    if alignment_model not in ALIGNMENT_MODELS:
        raise ValueError(f"alignment_model {alignment_model!r}: one of {ALIGNMENT_MODELS}")
    options = {"TN": dict(tn_max_step=5, min_length=4), "DP": dict(min_length=4), "HV": dict()}[alignment_model]
    candidates = candidates[: int(len(queries) * localize_per_query)]
    if alignment == "hip":
        if model is not None:
            raise ValueError("model= selects a VCSL-interface model; alignment='hip' runs its own kernel")
        from vsc.baseline.localization import (HipTNLocalizationCandidateScore, HipTNLocalizationMaxSim,
                                               HipVCSLLocalizationCandidateScore, HipVCSLLocalizationMaxSim)
        if score_normalization:
            if alignment_model == "TN":
                aligner = HipTNLocalizationMaxSim(queries, refs, similarity_bias=0.5, **options)
            else:
                aligner = HipVCSLLocalizationMaxSim(queries, refs, alignment_model, similarity_bias=0.5, **options)
        else:
            from vsc.baseline.score_normalization import normalize_videos
            if alignment_model == "TN":
                aligner = HipTNLocalizationCandidateScore(normalize_videos(queries), normalize_videos(refs), **options)
            else:
                aligner = HipVCSLLocalizationCandidateScore(normalize_videos(queries), normalize_videos(refs), alignment_model,
                                                            **options)
    elif score_normalization:
        aligner = VCSLLocalizationMaxSim(queries, refs, model_type=alignment_model, concurrency=16, similarity_bias=0.5,
                                         model=model, **options)
    else:
        from vsc.baseline.score_normalization import normalize_videos      # row-wise, a block of videos per device round trip
        aligner = VCSLLocalizationCandidateScore(normalize_videos(queries), normalize_videos(refs), model_type=alignment_model,
                                                 concurrency=16, model=model, **options)
    matches: List[Match] = []
    logger.info("Aligning %s candidate pairs", len(candidates))
    for i in range(0, len(candidates), 512):
        matches.extend(aligner.localize_all(candidates[i:i + 512]))
        logger.info("Aligned %d pairs of %d; %d predictions so far", min(i + 512, len(candidates)), len(candidates),
                    len(matches))
    return matches


def read_ground_truth_pairs(path: str) -> List[CandidatePair]:
    """(query_id, ref_id) pairs of a matching ground-truth csv (Match.read_csv + from_matches)."""
    import pandas as pd
    from vsc.metrics import format_video_id
    df = pd.read_csv(path)
    pairs = {(format_video_id(q, Dataset.QUERIES), format_video_id(r, Dataset.REFS))
             for q, r in zip(df.query_id, df.ref_id)}
    return [CandidatePair(q, r, 1.0) for q, r in sorted(pairs)]


def main(args) -> None:
    if os.path.exists(args.output_path) and not args.overwrite:
        raise Exception(f"Output path already exists: {args.output_path}. Do you want to --overwrite?")
    queries = load_features(args.query_features, Dataset.QUERIES)
    refs = load_features(args.ref_features, Dataset.REFS)
    os.makedirs(args.output_path, exist_ok=True)
    if args.score_norm_features:
        queries, refs = score_normalize(queries, refs, load_features(args.score_norm_features, Dataset.REFS),
                                        beta=1.2, device=getattr(args, "score_norm", "host"))   # (namespaces from before the option)
        store_features(os.path.join(args.output_path, "sn_queries.npz"), queries)
        store_features(os.path.join(args.output_path, "sn_refs.npz"), refs)
    candidates = search(queries, refs, selection=getattr(args, "candidates", "host"))
    candidate_file = os.path.join(args.output_path, "candidates.csv")
    CandidatePair.write_csv(candidates, candidate_file)
    logger.info("Candidates: %s", candidate_file)
    try:
        matches = localize_and_verify(queries, refs, candidates, score_normalization=bool(args.score_norm_features),
                                      alignment=args.alignment,
                                      alignment_model=getattr(args, "alignment_model", "TN"))   # (namespaces from before the option)
    except ImportError as exc:
        matches_file = None
        logger.warning("matches.csv not written: %s", exc)
    else:
        matches_file = os.path.join(args.output_path, "matches.csv")
        Match.write_csv(matches, matches_file)
        logger.info("Matches: %s", matches_file)
    if args.ground_truth:
        # the reference logs the canonical `.ap` (tied scores grouped), sscd_baseline.py:213-219
        uap_device = getattr(args, "uap", "host")                       # main() is also called with namespaces from before the option
        if uap_device not in UAPS:
            raise ValueError(f"uap {uap_device!r}: one of {UAPS}")
        uap = average_precision(read_ground_truth_pairs(args.ground_truth), candidates, device=uap_device)
        logger.info("Candidate uAP: %.4f", uap.ap)
        print(f"Candidate uAP: {uap.ap:.4f}")
        segment_metric = getattr(args, "segment_metric", "none")       # main() is also called with namespaces from before the option
        if segment_metric not in SEGMENT_METRICS:
            raise ValueError(f"segment_metric {segment_metric!r}: one of {SEGMENT_METRICS}")
        if segment_metric == "hip" and matches_file:
            # sscd_baseline.py:224-225 of the matching track: evaluate_matching_track on the file just written
            from vsc.metrics import evaluate_matching_track
            metrics = evaluate_matching_track(args.ground_truth, matches_file, uap=uap_device)
            logger.info("Matching track metric: %.4f", metrics.segment_ap.ap)
            logger.info("Matching track pairwise uAP: %.4f", metrics.pairwise_micro_ap.ap)
            print(f"Matching track metric: {metrics.segment_ap.ap:.4f}")
            print(f"Matching track pairwise uAP: {metrics.pairwise_micro_ap.ap:.4f}")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--query_features", required=True)
    ap.add_argument("--ref_features", required=True)
    ap.add_argument("--score_norm_features")
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--ground_truth")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--alignment", choices=ALIGNMENTS, default="vcsl",
                    help="temporal alignment of matches.csv: the reference's VCSL package (vcsl) or the HIP kernel (hip)")
    ap.add_argument("--alignment_model", choices=ALIGNMENT_MODELS, default="TN",
                    help="the alignment model (VCSL's model_type): temporal network (TN, the reference's choice), dynamic programming "
                         "(DP) or Hough voting (HV); with --alignment hip on the device, with --alignment vcsl handed to VCSL")
    ap.add_argument("--candidates", choices=CANDIDATES, default="host",
                    help="global top-k selection and video-pair grouping of candidates.csv: on the host (host) or in HIP (hip)")
    ap.add_argument("--score_norm", choices=SCORE_NORMS, default="host",
                    help="with --score_norm_features: the normalisation's arithmetic in numpy on the host (host) or on the device (hip: "
                         "vsc_column_var_f32 / vsc_score_norm_rows_f32 / vsc_score_norm_bias_f32; the same sn_*.npz, and the normalised "
                         "references stay on the device as the search's bank)")
    ap.add_argument("--segment_metric", choices=SEGMENT_METRICS, default="none",
                    help="with --ground_truth and a written matches.csv: the matching-track segment AP on the device (hip)")
    ap.add_argument("--uap", choices=UAPS, default="host",
                    help="with --ground_truth: the micro-AP (Candidate uAP and, with --segment_metric hip, the pairwise uAP) by the numpy "
                         "mirror on the host (host) or on the device in the reference's summation order (hip: vsc_uap_rank_f64 / "
                         "vsc_uap_curve_f64)")
    return ap


if __name__ == "__main__":
    logging.basicConfig(format="%(asctime)s %(levelname)-8s %(message)s", level=logging.INFO)
    main(build_parser().parse_args())
