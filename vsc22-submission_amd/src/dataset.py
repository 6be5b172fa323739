"""Frame sources for the extractor (reference: infer/src/dataset.py:101-153 D_vsc, and
infer/src/transform.py:37-42 vit_transform).  torchvision is not needed: Resize on a PIL image
is PIL's own bicubic resize, ToTensor is /255 and Normalize(0.5, 0.5) is 2x-1."""
from __future__ import annotations

import io
import os
from typing import List, Sequence
from zipfile import ZipFile

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence


def vit_transform(width: int, height: int):
    from PIL import Image

    def apply(img) -> torch.Tensor:
        img = img.convert("RGB").resize((height, width), Image.BICUBIC)   # Resize([w, h]) = (rows, cols)
        x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.0
        return (x - 0.5) / 0.5
    return apply


def vit_transform_u8(width: int, height: int):
    """The resize of ``vit_transform`` only: uint8 [H, W, 3].  ToTensor + Normalize(0.5, 0.5) then run inside the encoder's
    patchify kernel (HipEncoder / SwinHipEncoder take uint8 [n,H,W,C]) -- same descriptors, a quarter of the bytes."""
    from PIL import Image

    def apply(img) -> torch.Tensor:
        return torch.from_numpy(np.asarray(img.convert("RGB").resize((height, width), Image.BICUBIC), dtype=np.uint8).copy())
    return apply


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_transform(size: int = 224):
    """Resize(size, bicubic) on the short side + CenterCrop(size) + ToTensor + CLIP normalisation
    (infer/extract_query_feats.py:97-105, the video-score model's input)."""
    from PIL import Image
    mean = torch.tensor(CLIP_MEAN).view(3, 1, 1)
    std = torch.tensor(CLIP_STD).view(3, 1, 1)

    def apply(img) -> torch.Tensor:
        img = img.convert("RGB")
        w, h = img.size
        if w <= h:
            nw, nh = size, int(size * h / w)     # torchvision Resize(int): short side -> size, long side truncated
        else:
            nw, nh = int(size * w / h), size
        img = img.resize((nw, nh), Image.BICUBIC)
        left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
        img = img.crop((left, top, left + size, top + size))
        x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.0
        return (x - mean) / std
    return apply


def clip_transform_u8(size: int = 224):
    """Resize + CenterCrop of ``clip_transform`` only: uint8 [size, size, 3] (normalise with CLIP_MEAN / CLIP_STD on the GPU)."""
    from PIL import Image

    def apply(img) -> torch.Tensor:
        img = img.convert("RGB")
        w, h = img.size
        nw, nh = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
        img = img.resize((nw, nh), Image.BICUBIC)
        left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
        return torch.from_numpy(np.asarray(img.crop((left, top, left + size, top + size)), dtype=np.uint8).copy())
    return apply


def sscd_transform_u8(mode: str):
    """The VSC22 baseline's two inference transforms up to ToTensor (infer/vsc/baseline/inference_impl.py:33-54) as uint8 Pillow
    transforms: uint8 [H', W', 3]; ToTensor + Normalize(ImageNet mean / std) then run on the device inside the CNN encoder's stem
    (vsc_hip.cnn_config.IMAGENET_MEAN / IMAGENET_STD).
    ``resize_288``: torchvision's Resize(288) -- short side to 288, long side int(288 * long / short), bilinear; a frame whose short
    side is 288 already is returned as it is.  ``resize_320_center``: Resize(320), then CenterCrop(320) with torchvision's offsets
    int(round((extent - 320) / 2.0))."""
    from PIL import Image
    if mode not in SSCD_TRANSFORMS:
        raise ValueError(f"transforms must be one of {SSCD_TRANSFORMS}, not {mode!r}")
    size = 288 if mode == "resize_288" else 320

    def apply(img) -> torch.Tensor:
        img = img.convert("RGB")
        w, h = img.size
        nw, nh = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
        if (nw, nh) != (w, h):
            img = img.resize((nw, nh), Image.BILINEAR)
        if mode == "resize_320_center":
            left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
            img = img.crop((left, top, left + size, top + size))
        return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy())
    return apply


SSCD_TRANSFORMS = ("resize_288", "resize_320_center")   # --transforms of a CNN arch (InferenceTransforms of the baseline)


RESIZES = ("host", "hip")   # where decoded frames become model inputs: Pillow in the loader workers, or vsc_frame_inputs_u8


def check_resize(resize: str) -> str:
    if resize not in RESIZES:
        raise ValueError(f"resize must be one of {RESIZES}, not {resize!r}")
    return resize


def square_target(h: int, w: int, size: int):
    """The ops.frame_inputs target row (y0, y1, x0, x1, out_h, out_w, top, left, crop_h, crop_w) of ``vit_transform_u8(size, size)``
    on an h x w frame: the whole frame to size x size."""
    return (0, h, 0, w, size, size, 0, 0, size, size)


def clip_target(h: int, w: int, size: int = 224):
    """The target row of ``clip_transform_u8(size)`` on an h x w frame: short side to ``size`` (the long side truncated), then the
    centre window, whose offsets round half to even as Python's round does."""
    nw, nh = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
    left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
    return (0, h, 0, w, nh, nw, top, left, size, size)


DECODES = ("host", "hip")   # where the zips' jpgs are decoded: Pillow in the loader workers, or vsc_jpeg_decode_u8


def check_decode(decode: str, resize: str = "hip") -> str:
    """``decode`` if it is a known value; "hip" hands compressed bytes to the main process and so needs ``resize="hip"``"""
    if decode not in DECODES:
        raise ValueError(f"decode must be one of {DECODES}, not {decode!r}")
    if decode == "hip" and resize != "hip":
        raise ValueError("decode='hip' needs resize='hip': the frames it decodes are on the device, where vsc_frame_inputs_u8 resizes them")
    return decode


DECODE_SPLITS = ("none", "markers", "substreams", "all")   # --decode_split (vsc_hip.jpeg.SPLITS): how --decode hip cuts a frame into items


def check_decode_split(split: str, decode: str = "hip") -> str:
    """``split`` if it is a known value; anything but "none" cuts the frames that ``decode="hip"`` decodes and so needs it"""
    if split not in DECODE_SPLITS:
        raise ValueError(f"decode_split must be one of {DECODE_SPLITS}, not {split!r}")
    if split != "none" and decode != "hip":
        raise ValueError("decode_split needs decode='hip' (--decode hip): it is the device decoder whose frames it cuts into items")
    return split


DECODE_SCANS = ("host", "hip")   # --decode_scans: who decodes a jpg of several scans (progressive, one scan per component, Huffman table ids 2 and 3)


def check_decode_scans(scans: str, decode: str = "hip") -> str:
    """``scans`` if it is a known value; "hip" hands such files to the device decoder (vsc_jpeg_decode_scans_u8) and so needs ``decode="hip"``"""
    if scans not in DECODE_SCANS:
        raise ValueError(f"decode_scans must be one of {DECODE_SCANS}, not {scans!r}")
    if scans == "hip" and decode != "hip":
        raise ValueError("decode_scans='hip' needs decode='hip' (--decode hip): it is the device decoder that takes the files of several scans")
    return scans


class BytesVideo:
    """A video as its loader worker read it for ``--decode hip``: ``data`` uint8 [bytes], the jpg files one after the other,
    ``offsets`` int64 [S + 1] where each starts and ``records`` the vsc_hip.jpeg.Frame (with ``--decode_scans hip`` also ScanFrame)
    of each.  Every file has been accepted by
    the parser and all have one size (``shape`` = (S, H, W)).  ``restarts``: the CSR (int64 ptr [S + 1], int32 off) of the
    restart-marker offsets in every frame's segment (vsc_hip.jpeg.restart_rows), which ``--decode_split`` cuts frames at."""

    def __init__(self, data, offsets, records, restarts=None):
        self.data, self.offsets, self.records = data, offsets, records
        self.restarts = restarts if restarts is not None else (np.zeros(len(records) + 1, np.int64), np.zeros(0, np.int32))

    @property
    def shape(self):
        return len(self.records), self.records[0].height, self.records[0].width

    def files(self):
        raw = self.data.numpy()
        return [raw[a:b].tobytes() for a, b in zip(self.offsets[:-1].tolist(), self.offsets[1:].tolist())]


def bytes_video(files, warn=None, scans="host"):
    """The jpg files of one video -> a BytesVideo, or None where the video stays with Pillow as a whole: a file the parser
    refuses (``warn(message)`` is told why), frames of different sizes, no frames.  ``scans="hip"``: the parser is
    vsc_hip.jpeg.parse_scans, which also takes files of several scans."""
    from vsc_hip import jpeg
    data, offsets, records = jpeg.pack(files) if scans == "host" else jpeg.pack_scans(files)
    for i, r in enumerate(records):
        if isinstance(r, jpeg.Refusal):
            if warn is not None:
                warn(f"frame {i} stays with the host decoder: {r.reason} ({r.message})")
            return None
    if len({(r.height, r.width) for r in records}) != 1:
        return None
    return BytesVideo(torch.from_numpy(data), offsets, records, jpeg.restart_rows(files, records))


def decode_rgb(img) -> np.ndarray:
    """A decoded Pillow image as uint8 [H, W, 3], the array the transforms' ``img.convert("RGB")`` resizes."""
    return np.asarray(img.convert("RGB"), dtype=np.uint8)


class ZipFrames(torch.utils.data.Dataset):
    """One item = all frames of one video, read from <prefix>/<vid[-2:]>/<vid>.zip of jpgs."""

    def __init__(self, video_ids: Sequence[str], zip_prefix: str, transform, raw=False, decode_scans="host"):
        """``raw`` (``--resize hip``): the workers only decode -- an item is (uint8 [S, H, W, 3] at the zip's own resolution, video_id)
        for ``raw_collate``; a video whose frames differ in size is resized by ``transform`` here, as without ``raw``.
        ``raw="bytes"`` (``--decode hip``): the workers only read the zip members and parse their headers -- an item is
        (BytesVideo, video_id); a video with a frame the parser refuses is decoded here as a whole, as with ``raw=True``.
        ``decode_scans="hip"`` (with ``raw="bytes"``): the parser also takes files of several scans (vsc_hip.jpeg.parse_scans)."""
        self.zip_prefix, self.transform, self.raw = zip_prefix, transform, raw
        self.decode_scans = check_decode_scans(decode_scans, "hip" if raw == "bytes" else "host")
        self.host_decoded = 0                                 # with raw="bytes": the videos this object (in its own process) decoded with Pillow
        self.video_ids = [v for v in video_ids if os.path.exists(self._path(v))]

    def _path(self, vid):
        return "%s/%s/%s.zip" % (self.zip_prefix, vid[-2:], vid)

    def __len__(self):
        return len(self.video_ids)

    def __getitem__(self, i):
        from PIL import Image
        vid = self.video_ids[i]
        with ZipFile(self._path(vid), "r") as z:
            if self.raw:
                files = [z.read(n) for n in sorted(z.namelist())]
                if self.raw == "bytes":
                    video = bytes_video(files, scans=self.decode_scans)
                    if video is not None:
                        return video, vid
                    self.host_decoded += 1
                images = [Image.open(io.BytesIO(f)).convert("RGB") for f in files]
                if len({im.size for im in images}) == 1:
                    return torch.from_numpy(np.stack([decode_rgb(im) for im in images])), vid
                return torch.stack([self.transform(im) for im in images]), vid
            frames = [self.transform(Image.open(io.BytesIO(z.read(n)))) for n in sorted(z.namelist())]
        return torch.stack(frames), vid


class RaggedZipFrames(ZipFrames):
    """``ZipFrames`` for transforms that keep the aspect ratio (``sscd_transform_u8``): one item = (the video's transformed frames as
    a LIST of uint8 [H_i, W_i, 3], video_id) for ``raw_collate`` -- nothing is stacked here, so the frames of a video may differ in
    size (``src.extractor.extract_cnn_feat`` groups them by size)."""

    def __getitem__(self, i):
        from PIL import Image
        vid = self.video_ids[i]
        with ZipFile(self._path(vid), "r") as z:
            return [self.transform(Image.open(io.BytesIO(z.read(n)))) for n in sorted(z.namelist())], vid


class TensorFrames(torch.utils.data.Dataset):
    """Already decoded videos: a list of (frames [S,3,H,W] float32, video_id)."""

    def __init__(self, videos: List):
        self.videos = videos

    def __len__(self):
        return len(self.videos)

    def __getitem__(self, i):
        return self.videos[i]


def raw_collate(batch):
    """``ZipFrames(raw=True)``: the videos of a loader batch as they are, [(frames, video_id)] -- their frames differ in shape"""
    return list(batch)


def collate_fn(batch):
    frames, vids = zip(*batch)
    lengths = torch.tensor([f.shape[0] for f in frames])
    frames = pad_sequence(frames, batch_first=True, padding_value=0.0)
    mask = (torch.arange(frames.shape[1])[None, :] < lengths[:, None]).long()
    return frames, mask, vids
