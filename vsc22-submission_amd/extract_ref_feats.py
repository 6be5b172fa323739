"""Reference-descriptor extraction, one process per GPU (reference: infer/extract_ref_feats.py).

    python -m torch.distributed.run --nproc-per-node N extract_ref_feats.py \
        --checkpoint_path vit.pth --arch vit_b16_224 --zip_prefix ../data/jpg_zips \
        --input_file ../data/meta/train/train_ref_vids.txt --save_file outputs/train_refs

Same outputs: <save_file>.npz in the reference layout, videos sorted by id.  Videos shard over
ranks; each rank writes <save_file>_<rank>.npz, rank 0 merges (as the reference does).

``--resize hip``: the loader workers only decode; every video's frames are uploaded at the zip's resolution and resized to the
encoder's input on the GPU (vsc_frame_inputs_u8, PIL-exact: the same file).  The default, ``host``, resizes with Pillow in the
workers.

``--decode hip`` (with ``--resize hip``): the workers only read the zip members and parse the jpg headers; a loader batch's files
are uploaded compressed and decoded on the GPU (vsc_jpeg_decode_u8: Pillow's bytes, so the same file).  A video with a frame that
is not a baseline JPEG of a supported sampling is decoded by its worker as a whole.  The default, ``host``, decodes with Pillow.

``--arch sscd_resnet50 --weights_format sscd_torchvision --transforms resize_288|resize_320_center --sscd_l2 on|off``: the VSC22
baseline's descriptor model (infer/vsc/baseline).  Its frames keep their own size (the transforms are the baseline's, in the
workers); the frames of a loader batch are encoded per (H, W).  ``--resize hip`` / ``--decode hip`` are refused with a CNN arch:
those kernels resize bicubically to a square."""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from src.dataset import SSCD_TRANSFORMS, RaggedZipFrames, sscd_transform_u8
from src.dataset import DECODE_SCANS, DECODE_SPLITS, DECODES, RESIZES, ZipFrames, check_decode, check_decode_scans, check_decode_split, check_resize, collate_fn, raw_collate, vit_transform_u8
from src.extractor import extract_cnn_feat, extract_vsc_feat, extract_vsc_feat_raw
from vsc.storage import load_features, store_features
from src.model_zoo import DEFAULT_PRECISION, WEIGHT_FORMATS, load_encoder
from vsc_hip.cnn_config import CNN_PRESETS
from vsc_hip import distributed as vdist


def resize_of(args) -> str:
    """``args.resize``, "host" for a namespace built by hand from before the option; ValueError for an unknown value"""
    return check_resize(getattr(args, "resize", "host"))


def check_cnn_args(args) -> bool:
    """True for a CNN arch, whose options are checked here by name: ValueError before any device work"""
    if args.arch not in CNN_PRESETS:
        return False
    if resize_of(args) != "host":
        raise ValueError(f"--resize hip with the CNN arch {args.arch}: the device resize is bicubic-to-square only; use --transforms (Pillow in the workers)")
    if getattr(args, "decode", "host") != "host":
        raise ValueError(f"--decode hip with the CNN arch {args.arch}: it needs --resize hip, which a CNN arch refuses")
    if getattr(args, "transforms", "resize_288") not in SSCD_TRANSFORMS:
        raise ValueError(f"--transforms must be one of {SSCD_TRANSFORMS}, not {args.transforms!r}")
    if getattr(args, "sscd_l2", "on") not in ("on", "off"):
        raise ValueError(f"--sscd_l2 must be on or off, not {args.sscd_l2!r}")
    return True


def main(args):
    import torch.distributed as dist
    cnn = check_cnn_args(args)
    resize = resize_of(args)
    decode = check_decode(getattr(args, "decode", "host"), resize)
    decode_split = check_decode_split(getattr(args, "decode_split", "none"), decode)
    decode_scans = check_decode_scans(getattr(args, "decode_scans", "host"), decode)
    distributed = "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if distributed:
        dist.init_process_group(backend="nccl", init_method="env://", device_id=device)
    rank, world_size = vdist.world()
    model, image_size = load_encoder(args.arch, args.weights_format, args.checkpoint_path, args.max_batch,
                                     precision=getattr(args, "precision", DEFAULT_PRECISION), l2_normalize=getattr(args, "sscd_l2", "on") == "on")
    with open(args.input_file, encoding="utf-8") as f:
        vids = [x.strip() for x in f if x.strip()]
    lo, hi = vdist.shard_bounds(len(vids), rank, world_size)
    if cnn:
        data = RaggedZipFrames(vids[lo:hi], args.zip_prefix, sscd_transform_u8(getattr(args, "transforms", "resize_288")))
        loader = torch.utils.data.DataLoader(data, batch_size=args.batch_size, num_workers=getattr(args, "workers", 4), collate_fn=raw_collate)
        ids, feats, stamps = extract_cnn_feat(model, loader, device)
        return _write(args, ids, feats, stamps, rank, world_size, distributed)
    data = ZipFrames(vids[lo:hi], args.zip_prefix, vit_transform_u8(image_size, image_size), raw="bytes" if decode == "hip" else resize == "hip", decode_scans=decode_scans)   # uint8 to the GPU; normalised in patchify
    loader = torch.utils.data.DataLoader(data, batch_size=args.batch_size, num_workers=getattr(args, "workers", 4), collate_fn=raw_collate if resize == "hip" else collate_fn)
    if resize == "hip":
        from src.image_preprocess import HipDecode, HipResize
        ids, feats, stamps = extract_vsc_feat_raw(model, loader, device, image_size, HipResize(device), decoder=HipDecode(device, decode_split, decode_scans) if decode == "hip" else None)
    else:
        ids, feats, stamps = extract_vsc_feat(model, loader, device)
    _write(args, ids, feats, stamps, rank, world_size, distributed)


def _write(args, ids, feats, stamps, rank, world_size, distributed):
    import torch.distributed as dist
    np.savez(f"{args.save_file}_{rank}.npz", video_ids=ids, features=feats, timestamps=stamps)
    if distributed:
        dist.barrier()
    if rank == 0:
        parts = [np.load(f"{args.save_file}_{i}.npz") for i in range(world_size)]
        # a rank whose shard held no video (more ranks than videos, or all of its zips missing) wrote a (0, 0) feature
        # block and an empty float id array: leave such parts out of the merge
        parts = [p for p in parts if len(p["features"])] or parts[:1]
        np.savez(args.save_file + ".npz", video_ids=np.concatenate([p["video_ids"] for p in parts]),
                 features=np.concatenate([p["features"] for p in parts]),
                 timestamps=np.concatenate([p["timestamps"] for p in parts]))
        for i in range(world_size):
            os.remove(f"{args.save_file}_{i}.npz")
        store_features(args.save_file + ".npz", sorted(load_features(args.save_file + ".npz"), key=lambda v: v.video_id))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save_file", default="test_refs")
    ap.add_argument("--zip_prefix", default="")
    ap.add_argument("--input_file", default="test/test_reference.txt")
    ap.add_argument("--checkpoint_path", required=True)
    ap.add_argument("--arch", default="vit_b16_224", help="ViT preset (vsc_hip.config), Swin-V2 preset (vsc_hip.swin_config) or CNN preset (vsc_hip.cnn_config: sscd_resnet50)")
    ap.add_argument("--weights_format", default="hf_vit", choices=WEIGHT_FORMATS)
    ap.add_argument("--batch_size", type=int, default=2, help="videos per loader batch")
    ap.add_argument("--max_batch", type=int, default=None,
                    help="frames per encoder step; default: the backbone's tile-aligned batch (ViT-B/16: 332)")
    ap.add_argument("--precision", default=DEFAULT_PRECISION, choices=["fp16", "bf16"],
                    help="16-bit type of the encoder's MFMA operands (same speed; fp16 = 8 x smaller rounding, DESIGN.md 3a)")
    ap.add_argument("--resize", default="host", choices=RESIZES,
                    help="where decoded frames are resized to the encoder's input: Pillow in the loader workers, or on the device "
                         "(hip: the workers only decode; the same file)")
    ap.add_argument("--workers", type=int, default=4, help="loader worker processes (0: the main process reads and decodes the zips itself)")
    ap.add_argument("--decode", default="host", choices=DECODES,
                    help="where the zips' jpgs are decoded: Pillow in the loader workers, or on the device (hip, needs --resize hip: the "
                         "workers hand the compressed files on; the same file)")
    ap.add_argument("--decode_split", default="none", choices=DECODE_SPLITS,
                    help="with --decode hip (needed, and refused without it): decode in parallel inside a frame -- at its restart markers "
                         "(markers), as self-synchronising sub-streams of a frame without them (substreams) or both (all); the same "
                         "file.  Measured faster than one wave per frame at every call size from 40 to 1 024 frames, most at the 40 frames of one video (DESIGN 4.19)")
    ap.add_argument("--decode_scans", default="host", choices=DECODE_SCANS,
                    help="with --decode hip (needed, and refused without it): jpgs of several scans -- progressive, one scan per component, "
                         "Huffman table ids 2 and 3 -- are decoded on the device too (hip) instead of sending their whole video back to "
                         "Pillow in a loader worker (host); the same file.  With --decode_split such frames are one wave each")
    ap.add_argument("--transforms", default="resize_288", choices=SSCD_TRANSFORMS,
                    help="CNN arch only: the baseline's inference transform (Pillow, in the loader workers)")
    ap.add_argument("--sscd_l2", default="on", choices=["on", "off"],
                    help="CNN arch only: on = the original SSCD model's L2-normalised descriptor, off = the adapted model's raw projection")
    return ap


if __name__ == "__main__":
    main(build_parser().parse_args())
