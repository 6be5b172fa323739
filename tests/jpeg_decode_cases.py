"""The cases of the JPEG decoder's tests (CPU contract, emulated kernel, GPU entry): files written at test time by Pillow's encoder
from seeded arrays.  A case is one vsc_jpeg_decode_u8 call: a list of files.  ``files(name)`` are its bytes, ``pillow(name)`` what
the loader workers get today (``np.asarray(Image.open(f).convert("RGB"))``) and ``contract(name)`` the numpy contract's frames;
each is computed once per process and must not be modified.  ``call(files)`` packs a case into the operands of the entry."""
import functools
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "vsc22-submission_amd"))
sys.path.insert(0, HERE)

from vsc_hip import jpeg  # noqa: E402

SUB = {"444": 0, "422": 1, "420": 2}


def picture(seed, h, w, gray=False):
    """a smooth gradient with a few hard edges and some noise: every coefficient class occurs at moderate cost"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 37) % 256], axis=-1).astype(np.int32)
    base[(x // 5 + y // 7) % 3 == 0] //= 3
    out = np.clip(base + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    return out[:, :, 0] if gray else out


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def checker(h, w):
    y, x = np.mgrid[0:h, 0:w]
    c = (((x + y) & 1) * 255).astype(np.uint8)
    return np.stack([c, 255 - c, c], axis=-1)


def encode(arr, sampling="420", quality=75, **kw):
    buf = io.BytesIO()
    if arr.ndim == 2:
        Image.fromarray(arr, "L").save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(arr, "RGB").save(buf, "JPEG", quality=quality, subsampling=SUB[sampling], **kw)
    return buf.getvalue()


def _mixed70():
    """70 frames: every sampling class, sizes from 1 x 1 to 40 x 56, restart intervals in some, and three table sets: the encoder's
    default Huffman tables with quality 75 and 90 in the colour frames, quality 50 in the one-component ones"""
    sizes = [(1, 1), (3, 5), (8, 8), (16, 16), (17, 9), (9, 17), (24, 40), (33, 31), (40, 56), (7, 2)]
    out = []
    for i in range(70):
        h, w = sizes[i % len(sizes)]
        s = ("420", "422", "444", "gray")[(i // 2) % 4]
        q = 50 if s == "gray" else (75, 90)[i % 3 % 2]
        kw = {"restart_marker_blocks": 3} if i % 7 == 3 else {}
        out.append(encode(picture(1000 + i, h, w, gray=True), quality=q, **kw) if s == "gray" else encode(picture(1000 + i, h, w), s, q, **kw))
    return out


CASES = {}
for _h, _w in ((1, 1), (3, 5), (4, 4), (5, 3)):
    for _s in ("420", "422"):
        CASES[f"{_h}x{_w}_{_s}"] = functools.partial(lambda h, w, s: [encode(picture(h * 100 + w, h, w), s)], _h, _w, _s)
CASES.update({
    "8x8_444": lambda: [encode(picture(1, 8, 8), "444")],
    "8x8_gray": lambda: [encode(picture(2, 8, 8, gray=True))],
    "16x16_420": lambda: [encode(picture(3, 16, 16), "420")],
    "17x9_420": lambda: [encode(picture(4, 17, 9), "420")],
    "9x17_420": lambda: [encode(picture(5, 9, 17), "420")],
    "17x9_422": lambda: [encode(picture(6, 17, 9), "422")],
    "9x17_422": lambda: [encode(picture(7, 9, 17), "422")],
    "37x53_444": lambda: [encode(picture(8, 37, 53), "444")],
    "37x53_422": lambda: [encode(picture(9, 37, 53), "422")],
    "37x53_420": lambda: [encode(picture(10, 37, 53), "420")],
    "37x53_gray": lambda: [encode(picture(11, 37, 53, gray=True))],
    "noise_q5": lambda: [encode(noise(12, 33, 47), "420", 5)],
    "noise_q75": lambda: [encode(noise(13, 33, 47), "420", 75)],
    "noise_q100": lambda: [encode(noise(14, 33, 47), "420", 100), encode(noise(15, 24, 24), "444", 100)],
    "checker_q5": lambda: [encode(checker(33, 47), "420", 5)],
    "checker_q75": lambda: [encode(checker(33, 47), "422", 75)],
    "checker_q100": lambda: [encode(checker(33, 47), "444", 100), encode(checker(16, 24), "420", 100)],
    "64x48_restart_2_mcus": lambda: [encode(picture(16, 64, 48), "420", restart_marker_blocks=2)],
    "64x48_restart_mcu_row": lambda: [encode(picture(17, 64, 48), "420", restart_marker_rows=1), encode(picture(18, 64, 48), "444", restart_marker_rows=1)],
    "37x53_optimize": lambda: [encode(picture(19, 37, 53), "420", optimize=True), encode(picture(20, 37, 53, gray=True), optimize=True)],
    "360x640_420": lambda: [encode(picture(21, 360, 640), "420")],
    "mixed70": _mixed70,
    "empty": lambda: [],
    "five_small": lambda: [encode(picture(30 + i, 16 + 8 * i, 24), ("420", "444", "422", "420", "gray")[i]) if i < 4
                           else encode(picture(34, 48, 24, gray=True)) for i in range(5)],
})
BIG = ("360x640_420",)       # too many barriers for one OS thread per lane: contract and GPU only


def names(emulated=False):
    return [n for n in CASES if not (emulated and n in BIG)]


@functools.lru_cache(maxsize=None)
def files(name):
    return tuple(CASES[name]())


@functools.lru_cache(maxsize=None)
def pillow(name):
    return tuple(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files(name))


@functools.lru_cache(maxsize=None)
def contract(name):
    import jpeg_decode_contract
    return tuple(jpeg_decode_contract.decode(f) for f in files(name))


@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (bytes, the parser's reason)"""
    rgb = picture(40, 24, 32)
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").convert("CMYK").save(buf, "JPEG")
    whole = encode(rgb)
    return {"progressive": (encode(rgb, progressive=True), "progressive"), "cmyk": (buf.getvalue(), "components"),
            "cut_in_header": (whole[:whole.index(b"\xff\xc4") + 9], "truncated_header")}


@functools.lru_cache(maxsize=None)
def corrupt():
    """name -> bytes of a file whose header parses and whose scan is damaged (emulation and sanitizer runs only)"""
    whole = encode(picture(41, 40, 56), "420", 90)
    f = jpeg.parse(whole)
    third = f.seg_start + (f.seg_end - f.seg_start) // 3
    mid = f.seg_start + (f.seg_end - f.seg_start) // 2
    flipped = bytearray(whole)
    flipped[mid] ^= 0xFF
    rst = encode(picture(42, 64, 48), "420", restart_marker_blocks=2)
    at = rst.index(b"\xff\xd1", jpeg.parse(rst).seg_start)
    return {"scan_cut_at_a_third": whole[:third], "flipped_byte": bytes(flipped), "deleted_rst": rst[:at] + rst[at + 2:]}


def call(file_list, first_offset=0, gap=0):
    """-> (bytes uint8, frame table int64 [n, 10], table sets uint8 [s, TABLE_SET_BYTES], out_len, [(offset, h, w)]): every file
    parsed (all must be accepted), outputs packed from ``first_offset`` on with ``gap`` bytes between frames"""
    data, offsets, records = jpeg.pack(file_list)
    assert all(isinstance(r, jpeg.Frame) for r in records), [r for r in records if not isinstance(r, jpeg.Frame)]
    sets = jpeg.TableSets()
    outs, at = [], first_offset
    for r in records:
        outs.append((at, r.height, r.width))
        at += r.height * r.width * 3 + gap
    rows = jpeg.frame_rows(records, offsets[:-1].tolist(), [o[0] for o in outs], sets)
    tables = sets.array() if len(sets) else np.zeros((0, jpeg.TABLE_SET_BYTES), np.uint8)
    return data, rows, tables, at, outs
