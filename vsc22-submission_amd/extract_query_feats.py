"""Query-descriptor extraction with the backbone ensemble (reference: infer/extract_query_feats.py).

    python extract_query_feats.py --split test \
        --models swinv2_base_256:swin_ref:ckpt/swinv2_v115.pth swinv2_base_256:swin_ref:ckpt/swinv2_v107.pth \
                 swinv2_base_256:swin_ref:ckpt/swinv2_v106.pth vit_v68:timm_vit:ckpt/vit_v68.pth \
        --pca_model ckpt/pca_model.pkl --zip_prefix ../data/jpg_zips --input_file ../data/meta/test/query_ids.txt \
        --norm_refs outputs/train_refs.npz --output_dir outputs [--video_scores video_scores.csv] [--preprocess hip]

Outputs, as the reference: ``<output_dir>/<model name>/<split>_query.npz`` per backbone (:238-245) and
``<output_dir>/<split>_query_sn.npz`` after query score normalisation (:247-252).  The video-score gate
(CLIP ViT-L/14 [CLS] features -> ``MS`` head, :163-174) runs on the HIP path when ``--clip_checkpoint`` and
``--vsm_checkpoint`` (the state dicts torch2scripts.py traces) are given; otherwise scores are read from
``--video_scores`` (csv: video_id,score) and every video passes when neither is given.

``--preprocess hip`` adds the reference's query preprocessing (infer/src/image_preprocess.py ``image_process``, applied by
infer/src/dataset.py:82-88): static borders are cropped and stacked compositions split into views on the GPU
(src/image_preprocess.py), and every view's frames are encoded -- k views of n frames give k * n descriptor rows, timestamps
repeated view-major.  The video-score gate keeps the original frames.  The default, ``none``, encodes whole frames.

``--resize hip``: the loader workers only decode; every encoder input and the video-score input are made from the uploaded frames
on the GPU (vsc_frame_inputs_u8, PIL-exact: the same files), with ``--preprocess hip`` from the same upload as the views.  The
default, ``host``, resizes with Pillow in the workers.

``--decode hip`` (with ``--resize hip``): the workers only read the zip members and parse the jpg headers; each video's files are
uploaded compressed and decoded on the GPU (vsc_jpeg_decode_u8: Pillow's bytes, so the same files).  A video with a frame that is
not a baseline JPEG of a supported sampling is decoded by its worker as a whole.  The default, ``host``, decodes with Pillow."""
from __future__ import annotations

import argparse
import csv
import io
import os
from zipfile import ZipFile

import numpy as np
import torch

from src.dataset import CLIP_MEAN, CLIP_STD, DECODE_SCANS, DECODE_SPLITS, DECODES, RESIZES, bytes_video, check_decode, check_decode_scans, check_decode_split, check_resize, clip_transform_u8, decode_rgb, vit_transform_u8
from src.matching import calclualte_low_var_dim
from src.model_zoo import DEFAULT_PRECISION, load_encoder, parse_model_spec
from src.image_preprocess import HipViews, VIEW_DECISIONS
from src.query_pipeline import RAW_KEY, VideoScorer, run_query_videos
from src.query_postprocess import FRAME_FILTERS, HipPCA, SCORE_THRESHOLD, load_pca_model
from vsc.baseline.score_normalization import DEVICES as SCORE_NORMS, ScoreNormBank, query_score_normalize
from vsc.metrics import Dataset
from vsc.storage import load_features, store_features

NK, BETA = 1, 1.2  # extract_query_feats.py:56-57


class QueryVideos(torch.utils.data.Dataset):
    """One item = (video_id, {size: uint8 frames [S,size,size,3]}, timestamps): the jpgs of
    <prefix>/<vid[-2:]>/<vid>.zip decoded once and resized per input size (bicubic, as vit_transform / the CLIP
    transform do).  Frames stay uint8 until they are on the GPU: ToTensor + Normalize run inside the encoders'
    patchify kernels.  Decoding is the slow part of the whole pipeline, so main() reads this through a DataLoader with
    worker processes, as the reference does (extract_query_feats.py:138-140).
    ``preprocess="hip"``: the frames stay at the zip's own resolution, uint8 [S,H,W,3] under ``RAW_KEY`` (run_query_videos cuts
    and resizes the views on the GPU), next to the unchanged CLIP frames.  A video whose frames differ in size is resized here as
    with ``none``: the reference's preprocessing fails on it (np.stack) and leaves it unprocessed.
    ``resize="hip"``: the same raw frames and nothing else -- run_query_videos(resize="hip") makes every input, the CLIP frames
    included, on the GPU; a video whose frames differ in size is again resized here.
    ``decode="hip"`` (with ``resize="hip"``): the zip members are only read and their headers parsed -- the item carries a
    src.dataset.BytesVideo under ``RAW_KEY``; a video with a frame the parser refuses is decoded here as a whole.
    ``decode_scans="hip"`` (with ``decode="hip"``): the parser also takes files of several scans (vsc_hip.jpeg.parse_scans).
    ``host_decoded`` counts the videos this object decoded with Pillow."""

    def __init__(self, video_ids, zip_prefix, sizes, with_clip=False, preprocess="none", resize="host", decode="host", decode_scans="host"):
        assert preprocess in ("none", "hip"), preprocess
        self.zip_prefix, self.preprocess, self.resize = zip_prefix, preprocess, check_resize(resize)
        self.decode = check_decode(decode, self.resize)
        self.decode_scans = check_decode_scans(decode_scans, self.decode)
        self.host_decoded = 0
        self.video_ids = [v for v in video_ids if os.path.exists(self._path(v))]
        self.transforms = {s: vit_transform_u8(s, s) for s in sizes}
        if with_clip:
            self.transforms[VideoScorer.KEY] = clip_transform_u8(224)

    def _path(self, vid):
        return "%s/%s/%s.zip" % (self.zip_prefix, vid[-2:], vid)

    def __len__(self):
        return len(self.video_ids)

    def __getitem__(self, i):
        from PIL import Image
        vid = self.video_ids[i]
        with ZipFile(self._path(vid), "r") as z:
            files = [z.read(n) for n in sorted(z.namelist())]
        video = bytes_video(files, scans=self.decode_scans) if self.decode == "hip" else None
        if video is not None:
            n = video.shape[0]
            return vid, {RAW_KEY: video}, np.stack([np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32) + 1.0], axis=1)
        self.host_decoded += 1
        images = [Image.open(io.BytesIO(f)).convert("RGB") for f in files]
        # [start, end] seconds per frame at 1 fps, the layout the reference's FFmpeg reader yields (infer/src/dataset.py:97-102):
        # a video rejected by the score gate gets a [1, 2] placeholder, so every video's timestamps must be 2-D for
        # store_features to concatenate them
        n = len(images)
        stamps = np.stack([np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32) + 1.0], axis=1)
        if (self.preprocess == "hip" or self.resize == "hip") and len({im.size for im in images}) == 1:
            frames = {RAW_KEY: torch.from_numpy(np.stack([decode_rgb(im) for im in images]))}
            if VideoScorer.KEY in self.transforms and self.resize != "hip":
                frames[VideoScorer.KEY] = torch.stack([self.transforms[VideoScorer.KEY](im) for im in images])
            return vid, frames, stamps
        return vid, {s: torch.stack([t(im) for im in images]) for s, t in self.transforms.items()}, stamps


def zip_videos(video_ids, zip_prefix, sizes, with_clip=False, workers=0, preprocess="none", resize="host", decode="host", decode_scans="host"):
    data = QueryVideos(video_ids, zip_prefix, sizes, with_clip, preprocess, resize, decode, decode_scans)
    kw = {"prefetch_factor": 4} if workers > 0 else {}
    return torch.utils.data.DataLoader(data, batch_size=1, shuffle=False, num_workers=workers, collate_fn=lambda b: b[0], **kw)


def read_video_scores(path):
    if not path:
        return {}
    with open(path, newline="", encoding="utf-8") as f:
        rows = [r for r in csv.reader(f) if r and r[0] != "video_id"]
    return {r[0]: float(r[1]) for r in rows}


def resize_of(args) -> str:
    """``args.resize``, "host" for a namespace built by hand from before the option; ValueError for an unknown value"""
    return check_resize(getattr(args, "resize", "host"))


def check_models(models):
    """the parsed --models specs; a CNN arch is refused by name: the ensemble path is square-input only"""
    from vsc_hip.cnn_config import CNN_PRESETS
    specs = [parse_model_spec(s) for s in models]
    for arch, _, _ in specs:
        if arch in CNN_PRESETS:
            raise ValueError(f"--models: {arch} is a CNN arch; the query ensemble is square-input only (use extract_ref_feats.py --arch {arch})")
    return specs


def main(args):
    resize = resize_of(args)
    decode = check_decode(getattr(args, "decode", "host"), resize)
    decode_split = check_decode_split(getattr(args, "decode_split", "none"), decode)
    decode_scans = check_decode_scans(getattr(args, "decode_scans", "host"), decode)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    specs = check_models(args.models)
    encoders = [load_encoder(arch, fmt, path, args.max_batch, precision=args.precision) for arch, fmt, path in specs]
    pca = HipPCA(load_pca_model(args.pca_model))
    with open(args.input_file, encoding="utf-8") as f:
        vids = [x.strip() for x in f if x.strip()]
    scores = read_video_scores(args.video_scores)
    scorer = None
    if args.clip_checkpoint and args.vsm_checkpoint:
        from vsc_hip.video_score import VideoScoreHead, from_reference_state
        clip, _ = load_encoder("clip_vit_l14_224", "clip", args.clip_checkpoint, args.max_batch, u8_norm=(CLIP_MEAN, CLIP_STD),
                               precision=args.precision)
        from src.model_zoo import _state_dict      # a plain / training checkpoint or the TorchScript archive the reference ships (vsm.torchscript.pt)
        scorer = VideoScorer(clip, VideoScoreHead("vsm_roberta_base", from_reference_state(_state_dict(args.vsm_checkpoint))), device)
    videos = zip_videos(vids, args.zip_prefix, sorted({size for _, size in encoders}), with_clip=scorer is not None,
                        workers=args.workers, preprocess=args.preprocess, resize=resize, decode=decode, decode_scans=decode_scans)
    finals, per_model = run_query_videos(videos, encoders, pca.transform, scores, device, score_threshold=args.score_threshold,
                                         scorer=scorer, views=HipViews(device, getattr(args, "view_decisions", "host")) if args.preprocess == "hip" else None,
                                         frame_filter=getattr(args, "frame_filter", "host"),   # (a hand-built namespace from before the option)
                                         resize=resize, decode=decode, decode_split=decode_split, decode_scans=decode_scans)
    for i, (_, _, path) in enumerate(specs):
        key = os.path.split(path)[-1].split(".")[0]
        os.makedirs(os.path.join(args.output_dir, key), exist_ok=True)
        store_features(os.path.join(args.output_dir, key, f"{args.split}_query.npz"), [sub[i] for sub in per_model])
    if args.norm_refs:
        norm_refs = load_features(args.norm_refs, Dataset.REFS)
        score_norm = getattr(args, "score_norm", "host")   # main() is also called with namespaces built by hand, from before the option
        if score_norm == "hip":
            norm_refs = ScoreNormBank(norm_refs)           # uploaded once: the dimension, then the noise bank
        all_scores = {f.video_id: scores.get(f.video_id, 1.0) for f in finals}
        finals = query_score_normalize(finals, norm_refs, all_scores, args.score_threshold,
                                       calclualte_low_var_dim(norm_refs, device=score_norm), nk=NK, beta=BETA, device=score_norm)
    store_features(os.path.join(args.output_dir, f"{args.split}_query_sn.npz"), finals)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--split", default="test")
    ap.add_argument("--models", nargs="+", required=True, help="arch:weights_format:checkpoint_path, in concatenation order")
    ap.add_argument("--pca_model", required=True, help="the fitted PCA (mean_, components_, whiten, explained_variance_): .npz as concat_pca_sn.py --pca_fit hip writes it, else a pickled sklearn PCA")
    ap.add_argument("--zip_prefix", default="")
    ap.add_argument("--input_file", required=True, help="one query video id per line")
    ap.add_argument("--norm_refs", default="", help="score-normalisation reference descriptors (.npz)")
    ap.add_argument("--video_scores", default="", help="csv video_id,score from the video-score model")
    ap.add_argument("--clip_checkpoint", default="", help="CLIP ViT-L/14 visual tower state dict (video-score gate)")
    ap.add_argument("--vsm_checkpoint", default="", help="MS video-score head state dict (epoch_*.pth of train_vid_score)")
    ap.add_argument("--score_threshold", type=float, default=SCORE_THRESHOLD)
    ap.add_argument("--output_dir", default="outputs")
    ap.add_argument("--max_batch", type=int, default=None,
                    help="frames per encoder call; default: each backbone's tile-aligned batch (332 / 451 / 255 / 256)")
    ap.add_argument("--precision", default=DEFAULT_PRECISION, choices=["fp16", "bf16"],
                    help="16-bit type of the encoders' MFMA operands (same speed; fp16 = 8 x smaller rounding, DESIGN.md 3a)")
    ap.add_argument("--workers", type=int, default=6, help="decode / resize worker processes (the reference uses 6)")
    ap.add_argument("--preprocess", default="none", choices=["none", "hip"],
                    help="hip: crop static borders and split stacked views on the GPU before encoding (the reference's image_process)")
    ap.add_argument("--view_decisions", default="host", choices=VIEW_DECISIONS,
                    help="with --preprocess hip: the border / split decisions in numpy on the host (both maps are downloaded), or on "
                         "the device (hip: only the boxes come back; the same boxes, hence the same files)")
    ap.add_argument("--score_norm", default="host", choices=SCORE_NORMS,
                    help="with --norm_refs: the query score normalisation in numpy on the host, or on the device (hip; the same file)")
    ap.add_argument("--frame_filter", default="host", choices=FRAME_FILTERS,
                    help="the near-duplicate frame filter in numpy on the host, or on the device (hip: the similarity matrices are not "
                         "downloaded); the same files wherever a video's frame means are pairwise distinct -- equal means are visited in "
                         "descending index on the device and in numpy's unspecified order on the host")
    ap.add_argument("--resize", default="host", choices=RESIZES,
                    help="where decoded frames become model inputs: Pillow in the loader workers, or on the device (hip: the workers "
                         "only decode, one kernel call per video makes every encoder input and the video-score input; the same files)")
    ap.add_argument("--decode", default="host", choices=DECODES,
                    help="where the zips' jpgs are decoded: Pillow in the loader workers, or on the device (hip, needs --resize hip: the "
                         "workers hand the compressed files on; the same files)")
    ap.add_argument("--decode_split", default="none", choices=DECODE_SPLITS,
                    help="with --decode hip (needed, and refused without it): decode in parallel inside a frame -- at its restart markers "
                         "(markers), as self-synchronising sub-streams of a frame without them (substreams) or both (all); the same "
                         "files.  Measured faster than one wave per frame at every call size from 40 to 1 024 frames, most at the 40 frames of one video (DESIGN 4.19)")
    ap.add_argument("--decode_scans", default="host", choices=DECODE_SCANS,
                    help="with --decode hip (needed, and refused without it): jpgs of several scans -- progressive, one scan per component, "
                         "Huffman table ids 2 and 3 -- are decoded on the device too (hip) instead of sending their whole video back to "
                         "Pillow in a loader worker (host); the same files.  With --decode_split such frames are one wave each")
    return ap


if __name__ == "__main__":
    main(build_parser().parse_args())
