"""The cases of the multi-scan JPEG decoder's tests (CPU contract, emulated kernel, GPU entry).  A case is one file.  Pillow's encoder
writes the progressive ones at test time from seeded arrays: every size x sampling x quality x content of SIZES, SAMPLINGS, QUALITIES
and CONTENTS, plus optimised tables (custom tables per scan) and restart intervals.  What Pillow cannot write is made here from the
coefficients of a Pillow file by ``write_scans`` (a sequential Huffman encoder in a dozen lines): sequential files of one scan per
component, with a DHT redefined between scans, and -- by patching a header -- Huffman table ids 2 and 3.  ``pillow(name)`` is
``np.asarray(Image.open(f).convert("RGB"))`` of the same file, ``contract(name)`` the numpy contract's frame; each is computed once
per process and must not be modified.  ``damaged()`` are fixed files whose scans are broken, ``refused()`` files the parser refuses."""
import functools
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_decode_cases as single  # noqa: E402
import jpeg_decode_contract as base  # noqa: E402
import jpeg_scans_contract as contract_  # noqa: E402
from jpeg_decode_contract import jpeg  # noqa: E402

SIZES = ((1, 1), (8, 8), (13, 17), (16, 16), (33, 47), (48, 64), (120, 200))
SAMPLINGS = ("gray", "444", "422", "420")
QUALITIES = (30, 75, 95)
CONTENTS = ("noise", "ramp", "constant")


def content(kind, seed, h, w):
    """noise: dense coefficients and long runs of correction bits; ramp: EOBRUNs over many blocks; constant: DC only"""
    if kind == "noise":
        return single.noise(seed, h, w)
    if kind == "constant":
        return np.full((h, w, 3), (90, 160, 33), np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(h + w - 2, 1)], axis=-1).astype(np.uint8)


def encode(arr, sampling, quality, **kw):
    return single.encode(arr[:, :, 0] if sampling == "gray" else arr, "420" if sampling == "gray" else sampling, quality, **kw)


def _grid(h, w, s, q, kind, **kw):
    return encode(content(kind, h * 1000 + w * 10 + q, h, w), s, q, progressive=True, **kw)


CASES = {}
for _h, _w in SIZES:
    for _s in SAMPLINGS:
        for _q in QUALITIES:
            for _kind in CONTENTS:
                CASES[f"{_h}x{_w}_{_s}_q{_q}_{_kind}"] = functools.partial(_grid, _h, _w, _s, _q, _kind)
for _h, _w in ((13, 17), (33, 47), (48, 64)):
    for _s in SAMPLINGS:
        CASES[f"{_h}x{_w}_{_s}_optimize"] = functools.partial(_grid, _h, _w, _s, 75, "noise", optimize=True)
        CASES[f"{_h}x{_w}_{_s}_optimize_ramp"] = functools.partial(_grid, _h, _w, _s, 75, "ramp", optimize=True)
        CASES[f"{_h}x{_w}_{_s}_restart_3_blocks"] = functools.partial(_grid, _h, _w, _s, 75, "noise", restart_marker_blocks=3)
        CASES[f"{_h}x{_w}_{_s}_restart_row"] = functools.partial(_grid, _h, _w, _s, 75, "ramp", restart_marker_rows=1)


# ---- files Pillow cannot write -----------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc, self.n = self.acc << length | code, self.n + length
        while self.n >= 8:
            byte = self.acc >> (self.n - 8) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def codes(bits, vals):
    """a Huffman table -> {symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(int(bits[length - 1])):
            out[int(vals[k])] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def magnitude(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def encode_block(w, zz, pred, dc, ac):
    """one block (64 coefficients in zigzag order) of a sequential scan"""
    s, x = magnitude(int(zz[0]) - pred)
    w.put(*dc[s])
    if s:
        w.put(x, s)
    run = 0
    last = max([k for k in range(1, 64) if zz[k]], default=0)
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            run -= 16
        s, x = magnitude(int(zz[k]))
        w.put(*ac[run << 4 | s])
        w.put(x, s)
        run = 0
    if last < 63:
        w.put(*ac[0])
    return int(zz[0])


def dht(tc, th, bits, vals):
    n = int(np.sum(bits))
    return b"\xff\xc4" + (19 + n).to_bytes(2, "big") + bytes([tc << 4 | th]) + bytes(bits.tolist()) + bytes(vals[:n].tolist())


def write_scans(whole, redefine=False):
    """a baseline Pillow file of three components -> the same coefficients as a sequential file of one scan per component (Y with
    the tables DC0 / AC0).  Cb and Cr use DC1 / AC1; with ``redefine`` a DHT in front of the Cb scan re-defines DC0 / AC0 as the
    chroma tables instead and both chroma scans name table 0."""
    f = jpeg.parse(whole)
    assert isinstance(f, jpeg.Frame) and len(f.comp_tables) == 3
    coef = base.coefficients(f, whole)
    _, huff = base.tables_of(f.tables)
    enc = [codes(*h) for h in huff]
    _, _, _, _, comps = contract_.geometry(jpeg.as_scan_frame(f))
    sos = whole.rindex(b"\xff\xda", 0, f.seg_start)
    out = [whole[:sos]]
    for c in range(3):
        if c == 1 and redefine:
            out += [dht(0, 0, *huff[1]), dht(1, 0, *huff[3])]
        t = 0 if c == 0 or redefine else 1
        w, pred = BitWriter(), 0
        for by in range(comps[c][3]):
            for bx in range(comps[c][2]):
                pred = encode_block(w, coef[c][by, bx][jpeg.ZIGZAG], pred, enc[0 if c == 0 else 1], enc[2 if c == 0 else 3])
        out += [b"\xff\xda\x00\x08\x01" + bytes([c + 1, t << 4 | t, 0, 63, 0]), w.flush()]
    return b"".join(out) + b"\xff\xd9"


def table_ids_2_3(whole):
    """a baseline Pillow file with its Huffman tables 0 and 1 renamed 2 and 3, in the DHT segments and in the scan header"""
    f = jpeg.parse(whole)
    a = bytearray(whole)
    at = 2
    while at < f.seg_start:
        m, length = a[at + 1], a[at + 2] << 8 | a[at + 3]
        if m == 0xC4:
            k = at + 4
            while k < at + 2 + length:
                a[k] += 2
                k += 17 + sum(a[k + 1:k + 17])
        elif m == 0xDA:
            for c in range(a[at + 4]):
                a[at + 6 + 2 * c] += 0x22
        at += 2 + length
    return bytes(a)


def _handmade(kind, h, w, s, seed):
    whole = single.encode(single.picture(seed, h, w), s, 80)
    return table_ids_2_3(whole) if kind == "ids" else write_scans(whole, redefine=kind == "redefine")


HANDMADE = {}
for _i, (_h, _w) in enumerate(((13, 17), (48, 64), (33, 47))):
    for _s in ("444", "422", "420"):
        HANDMADE[f"{_h}x{_w}_{_s}_one_scan_per_component"] = functools.partial(_handmade, "plain", _h, _w, _s, 500 + _i)
HANDMADE["33x47_420_table_ids_2_3"] = functools.partial(_handmade, "ids", 33, 47, "420", 510)
HANDMADE["16x16_444_table_ids_2_3"] = functools.partial(_handmade, "ids", 16, 16, "444", 511)
HANDMADE["33x47_420_dht_redefined"] = functools.partial(_handmade, "redefine", 33, 47, "420", 512)
HANDMADE["13x17_422_dht_redefined"] = functools.partial(_handmade, "redefine", 13, 17, "422", 513)
CASES.update(HANDMADE)


def names():
    return list(CASES)


@functools.lru_cache(maxsize=None)
def file(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def pillow(name):
    return np.asarray(Image.open(io.BytesIO(file(name))).convert("RGB"))


@functools.lru_cache(maxsize=None)
def contract(name):
    return contract_.decode(file(name))


def twin(name):
    """the same image saved non-progressively at the same quality and sampling (grid cases only)"""
    size, s, q, kind = name.split("_")
    h, w = (int(v) for v in size.split("x"))
    return encode(content(kind, h * 1000 + w * 10 + int(q[1:]), h, w), s, int(q[1:]))


GRID = [n for n in CASES if len(n.split("_")) == 4 and n.split("_")[2][0] == "q"]


# ---- scans of a file as pieces -----------------------------------------------------------------------------------------------------
def pieces(whole):
    """-> (the bytes in front of the first scan's tables, [per scan: its DHT / DRI segments, header and data], the rest): a
    progressive Pillow file puts the tables a scan needs directly in front of it"""
    a = np.frombuffer(whole, np.uint8)
    at, head_end, start, out = 2, None, None, []
    while True:
        m = whole[at + 1]
        if m == 0xD9:
            break
        length = whole[at + 2] << 8 | whole[at + 3]
        if m in (0xC4, 0xDD) and start is None and head_end is not None:
            start = at
        if m in (0xC0, 0xC1, 0xC2):
            head_end = at + 2 + length
        if m == 0xDA:
            end, _ = jpeg.scan_end(a, at + 2 + length)
            out.append(whole[start if start is not None else at:end])
            at, start = end, None
            continue
        at += 2 + length
    first = len(whole) - len(whole[at:]) - sum(len(p) for p in out)
    return whole[:first], out, whole[at:]


@functools.lru_cache(maxsize=None)
def _progressive_420():
    return encode(content("noise", 77, 48, 64), "420", 75, progressive=True)


@functools.lru_cache(maxsize=None)
def refused():
    """name -> (bytes, parse_scans' reason, parse's refusal today)"""
    whole = _progressive_420()
    head, scans, tail = pieces(whole)
    assert len(scans) == 10 and head + b"".join(scans) + tail == whole
    today = jpeg.Refusal("progressive", "progressive DCT (SOF2)")
    sixth = bytearray(scans[5])
    assert sixth[sixth.index(b"\xff\xda") + 9] == 0x21       # Y, 1 .. 63, Ah 2, Al 1 -> Ah 1, Al 0
    sixth[sixth.index(b"\xff\xda") + 9] = 0x10
    cut = len(head) + sum(len(s) for s in scans[:3]) + len(scans[3]) - 7
    plain = single.encode(single.picture(40, 24, 32))
    sof = plain.index(b"\xff\xc0")
    arith = plain[:sof + 1] + b"\xc9" + plain[sof + 2:]
    twelve = plain[:sof + 4] + b"\x0c" + plain[sof + 5:]
    cmyk = single.refusals()["cmyk"][0]
    return {
        "ac_before_dc": (head + scans[1] + scans[0] + b"".join(scans[2:]) + tail, "scan_script", today),
        "ah_is_not_the_previous_al": (head + b"".join(scans[:5]) + bytes(sixth) + b"".join(scans[6:]) + tail, "scan_script", today),
        "band_left_at_al_1": (head + b"".join(scans[:9]) + tail, "incomplete_scans", today),
        "cut_in_fourth_scan": (whole[:cut], "truncated_scans", today),
        "arithmetic": (arith, "arithmetic", jpeg.Refusal("arithmetic", "arithmetic coding (SOF9)")),
        "twelve_bit": (twelve, "precision", jpeg.Refusal("precision", "12-bit samples")),
        "cmyk": (cmyk, "components", jpeg.Refusal("components", "4 components")),
    }


@functools.lru_cache(maxsize=None)
def damaged():
    """name -> (bytes, the contract's status): fixed files whose headers and scan script pass the parser and whose scans are broken"""
    whole = _progressive_420()
    head, scans, tail = pieces(whole)
    out = {}
    # a flipped bit in byte 20 of the last AC-refine scan (Y, 1 .. 63, Ah 1, Al 0): the symbols behind it run out of zero coefficients
    s = bytearray(scans[9])
    s[s.index(b"\xff\xda") + 10 + 20] ^= 0x10
    out["flipped_bit_in_ac_refine"] = head + b"".join(scans[:9]) + bytes(s) + tail
    # the third scan (Cr, AC first) shortened by its last byte
    out["scan_shortened_by_one_byte"] = head + b"".join(scans[:2]) + scans[2][:-1] + b"".join(scans[3:]) + tail
    # an EOBRUN that runs past the last block: a smooth gray 16 x 16 image's AC scan is one EOBRUN of 4 blocks; its image made 8 x 16
    ramp = encode(content("constant", 1, 16, 16), "gray", 75, progressive=True)
    sof = ramp.index(b"\xff\xc2")
    out["eobrun_past_the_last_block"] = ramp[:sof + 5] + b"\x00\x08" + ramp[sof + 7:]
    # RST1 where RST0 belongs, in the first scan
    rst = encode(content("noise", 78, 48, 64), "420", 75, progressive=True, restart_marker_blocks=2)
    at = rst.index(b"\xff\xd0", jpeg.parse_scans(rst).scans[0].seg_start)
    out["wrong_rst"] = rst[:at + 1] + b"\xd1" + rst[at + 2:]
    result = {}
    for name, data in out.items():
        frame = jpeg.parse_scans(data)
        assert isinstance(frame, jpeg.ScanFrame), (name, frame)
        result[name] = (data, contract_.decode_frame(frame, data)[1])
    return result


def call(file_list, first_offset=0, gap=0):
    """-> (bytes uint8, frame table, scan table, scan ptr, table sets uint8 [s, SCAN_TABLE_SET_BYTES], out_len, [(offset, h, w)])"""
    data, offsets, records = jpeg.pack_scans(file_list)
    assert all(isinstance(r, (jpeg.Frame, jpeg.ScanFrame)) for r in records), [r for r in records if isinstance(r, jpeg.Refusal)]
    sets = jpeg.ScanTableSets()
    outs, at = [], first_offset
    for r in records:
        outs.append((at, r.height, r.width))
        at += r.height * r.width * 3 + gap
    rows, srows, ptr = jpeg.scan_rows(records, offsets[:-1].tolist(), [o[0] for o in outs], sets)
    tables = sets.array() if len(sets) else np.zeros((0, jpeg.SCAN_TABLE_SET_BYTES), np.uint8)
    return data, rows, srows, ptr, tables, at, outs
