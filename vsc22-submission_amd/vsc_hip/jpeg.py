"""Header parser of ``--decode hip`` (vsc_jpeg_decode_u8, csrc/jpeg_decode.hip): numpy only, and nothing here opens the GPU --
the loader workers call it.  ``parse(data)`` reads the markers of one JPEG file up to its scan and returns either a ``Frame``
(what the device needs to decode it: size, sampling class, the tables each component uses, the restart interval, the byte range of
the entropy-coded segment, and the content of its tables as one fixed-size ``table set``) or a ``Refusal`` whose ``reason`` names
why the file stays with Pillow.  Nothing is approximated: what the device path cannot decode to Pillow's bytes is refused.

``TableSets`` de-duplicates table sets by content (all frames an encoder wrote with its default tables share one), and
``frame_rows`` packs the frame table of one vsc_jpeg_decode_u8 call.  The formats are those of include/vsc_hip.h.

``parse_scans(data)`` is the parser of ``--decode_scans hip`` (vsc_jpeg_decode_scans_u8, csrc/jpeg_scans.hip): the same ``Frame``
where ``parse`` accepts, a ``ScanFrame`` -- the scan list with the tables and the restart interval in force at every scan -- for a
progressive file, a sequential file of several scans and Huffman table ids 0 .. 3, a ``Refusal`` for everything else; ``scan_rows``
packs the frame and scan tables of one call.  ``parse`` itself refuses what it always refused."""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple, Union

import numpy as np

# sampling classes
GRAY, S444, S422, S420 = 0, 1, 2, 3
SAMPLING_NAMES = ("gray", "4:4:4", "4:2:2", "4:2:0")
MCU_SIDE = ((8, 8), (8, 8), (8, 16), (16, 16))       # (rows, columns) of luma one MCU covers, per class

# one table set: uint16 quant[4][64] (little endian, in the file's zigzag order), uint8 bits[4][16] and uint8 vals[4][256] of the
# Huffman tables DC0, DC1, AC0, AC1, then one byte of quantisation tables present (bit = table id), one of Huffman tables present
# (bit = 2 * class + id) and six bytes of zero
TABLE_SET_BYTES = 512 + 64 + 1024 + 8
FRAME_ROW = 10                                        # int64 per frame of the call's frame table
MAX_SIDE = 16384                                      # vsc_jpeg_decode_u8 takes frames up to this many pixels a side

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63], dtype=np.int32)                # natural (row-major) position of the k-th coefficient of a block


class Frame(NamedTuple):
    height: int
    width: int
    sampling: int                                  # GRAY, S444, S422 (h2v1) or S420 (h2v2)
    comp_tables: Tuple[Tuple[int, int, int], ...]  # per component: (quantisation table, DC Huffman table, AC Huffman table)
    restart: int                                   # MCUs per restart interval, 0: none
    seg_start: int                                 # the entropy-coded segment is data[seg_start:seg_end]: from behind the SOS header to the
    seg_end: int                                   # marker that ends the scan (EOI), or to the end of a file that has none
    tables: bytes                                  # TABLE_SET_BYTES

    @property
    def comp_word(self) -> int:
        """the frame row's component word: byte c = quantisation table | DC table << 2 | AC table << 3 of component c"""
        return sum((tq | td << 2 | ta << 3) << (8 * c) for c, (tq, td, ta) in enumerate(self.comp_tables))


class Refusal(NamedTuple):
    reason: str                                    # one of REASONS
    message: str


REASONS = ("not_jpeg", "truncated_header", "progressive", "arithmetic", "lossless", "hierarchical", "precision", "components", "adobe_rgb",
           "rgb_component_ids", "sampling", "multiple_scans", "missing_tables", "quant16", "huffman_table_id", "bad_header", "size")

_SOF_REFUSED = {0xC2: ("progressive", "progressive DCT (SOF2)"), 0xC3: ("lossless", "lossless (SOF3)"),
                0xC5: ("hierarchical", "differential sequential (SOF5)"), 0xC6: ("hierarchical", "differential progressive (SOF6)"),
                0xC7: ("hierarchical", "differential lossless (SOF7)"), 0xC9: ("arithmetic", "arithmetic coding (SOF9)"),
                0xCA: ("arithmetic", "arithmetic progressive (SOF10)"), 0xCB: ("arithmetic", "arithmetic lossless (SOF11)"),
                0xCD: ("arithmetic", "differential arithmetic (SOF13)"), 0xCE: ("arithmetic", "differential arithmetic (SOF14)"),
                0xCF: ("arithmetic", "differential arithmetic (SOF15)")}


def scan_end(a: np.ndarray, start: int) -> Tuple[int, int]:
    """(position, marker) of the first marker behind ``start`` that is neither a stuffed zero, a fill byte nor RSTn;
    (len(a), -1) when the data ends first"""
    ff = np.flatnonzero(a[start:len(a) - 1] == 0xFF) + start
    nxt = a[ff + 1]
    ends = ff[(nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    if len(ends) == 0:
        return len(a), -1
    return int(ends[0]), int(a[ends[0] + 1])


def parse(data) -> Union[Frame, Refusal]:
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    n = len(a)
    if n < 4 or a[0] != 0xFF or a[1] != 0xD8:
        return Refusal("not_jpeg", "no SOI marker")
    quant = np.zeros((4, 64), np.uint16)
    bits = np.zeros((4, 16), np.uint8)
    vals = np.zeros((4, 256), np.uint8)
    qmask = hmask = 0
    sof = None
    restart = 0
    jfif = False
    adobe = None
    pos = 2
    while True:
        if pos + 2 > n:
            return Refusal("truncated_header", "the file ends before its scan")
        if a[pos] != 0xFF:
            return Refusal("bad_header", f"byte {int(a[pos]):#x} at {pos} where a marker should be")
        m = int(a[pos + 1])
        if m == 0xFF:                                 # a fill byte
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:            # TEM, RSTn: no length
            pos += 2
            continue
        if m == 0xD9:
            return Refusal("truncated_header", "EOI before any scan")
        if pos + 4 > n:
            return Refusal("truncated_header", "the file ends inside a marker segment")
        length = int(a[pos + 2]) << 8 | int(a[pos + 3])
        if length < 2:
            return Refusal("bad_header", f"marker {m:#x} with length {length}")
        if pos + 2 + length > n:
            return Refusal("truncated_header", f"the file ends inside the segment of marker {m:#x}")
        seg = a[pos + 4:pos + 2 + length]
        if m in _SOF_REFUSED:
            return Refusal(*_SOF_REFUSED[m])
        if m == 0xCC:
            return Refusal("arithmetic", "arithmetic conditioning (DAC)")
        if m in (0xC0, 0xC1):
            if sof is not None:
                return Refusal("hierarchical", "a second frame header")
            if len(seg) < 6 or len(seg) < 6 + 3 * int(seg[5]):
                return Refusal("bad_header", "short SOF segment")
            sof = (int(seg[0]), int(seg[1]) << 8 | int(seg[2]), int(seg[3]) << 8 | int(seg[4]),
                   [(int(seg[6 + 3 * c]), int(seg[7 + 3 * c]) >> 4, int(seg[7 + 3 * c]) & 15, int(seg[8 + 3 * c])) for c in range(int(seg[5]))])
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = int(seg[at]) >> 4, int(seg[at]) & 15
                if pq != 0:
                    return Refusal("quant16", "a 16-bit quantisation table")
                if tq > 3 or at + 65 > len(seg):
                    return Refusal("bad_header", "bad DQT segment")
                quant[tq] = seg[at + 1:at + 65]
                qmask |= 1 << tq
                at += 65
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                tc, th = int(seg[at]) >> 4, int(seg[at]) & 15
                if tc > 1 or at + 17 > len(seg):
                    return Refusal("bad_header", "bad DHT segment")
                if th > 1:
                    return Refusal("huffman_table_id", f"Huffman table id {th} (0 and 1 are taken)")
                count = int(seg[at + 1:at + 17].sum())
                if count > 256 or at + 17 + count > len(seg):
                    return Refusal("bad_header", "bad DHT segment")
                t = 2 * tc + th
                bits[t] = seg[at + 1:at + 17]
                vals[t] = 0
                vals[t, :count] = seg[at + 17:at + 17 + count]
                hmask |= 1 << t
                at += 17 + count
        elif m == 0xDD:
            if len(seg) < 2:
                return Refusal("bad_header", "short DRI segment")
            restart = int(seg[0]) << 8 | int(seg[1])
        elif m == 0xE0:
            jfif = jfif or (len(seg) >= 5 and bytes(seg[:5]) == b"JFIF\0")
        elif m == 0xEE:
            if len(seg) >= 12 and bytes(seg[:5]) == b"Adobe":
                adobe = int(seg[11])
        elif m == 0xDA:
            break
        pos += 2 + length

    if sof is None:
        return Refusal("bad_header", "a scan without a frame header")
    precision, height, width, comps = sof
    if precision != 8:
        return Refusal("precision", f"{precision}-bit samples")
    if len(comps) not in (1, 3):
        return Refusal("components", f"{len(comps)} components")
    if height < 1 or width < 1 or height > MAX_SIDE or width > MAX_SIDE:
        return Refusal("size", f"{height} x {width} pixels (1 .. {MAX_SIDE} a side; a height of 0 is set by a DNL marker)")
    if len(comps) == 1:
        sampling = GRAY
    else:
        if adobe is not None and adobe == 0:
            return Refusal("adobe_rgb", "Adobe APP14 transform 0: the three components are RGB")
        if adobe is None and not jfif and tuple(c[0] for c in comps) == (82, 71, 66):
            return Refusal("rgb_component_ids", "components named R, G, B without a JFIF or Adobe marker")
        fac = tuple((c[1], c[2]) for c in comps)
        if fac[1:] != ((1, 1), (1, 1)) or fac[0] not in ((1, 1), (2, 1), (2, 2)):
            return Refusal("sampling", f"sampling factors {fac}")
        sampling = {(1, 1): S444, (2, 1): S422, (2, 2): S420}[fac[0]]
    ns = int(seg[0]) if len(seg) else 0
    if len(seg) < 1 + 2 * ns + 3:
        return Refusal("bad_header", "short SOS segment")
    if ns != len(comps):
        return Refusal("multiple_scans", f"a scan of {ns} of the {len(comps)} components")
    tables = []
    for c in range(ns):
        cs, tdta = int(seg[1 + 2 * c]), int(seg[2 + 2 * c])
        if cs != comps[c][0]:
            return Refusal("bad_header", "the scan lists the components in another order than the frame")
        td, ta = tdta >> 4, tdta & 15
        if td > 1 or ta > 1:
            return Refusal("huffman_table_id", f"Huffman table ids {td}, {ta} (0 and 1 are taken)")
        tq = comps[c][3]
        if tq > 3 or not (qmask >> tq & 1) or not (hmask >> td & 1) or not (hmask >> (2 + ta) & 1):
            return Refusal("missing_tables", f"component {c} uses a table the file does not define")
        tables.append((tq, td, ta))
    ss, se, ahal = (int(v) for v in seg[1 + 2 * ns:4 + 2 * ns])
    if (ss, se, ahal) != (0, 63, 0):
        return Refusal("progressive", f"a scan of coefficients {ss} .. {se}, approximation {ahal:#x}")
    seg_start = pos + 2 + length
    seg_end, marker = scan_end(a, seg_start)
    if marker not in (-1, 0xD9):
        return Refusal("multiple_scans", f"marker {marker:#x} follows the scan")
    blob = quant.astype("<u2").tobytes() + bits.tobytes() + vals.tobytes() + bytes([qmask, hmask, 0, 0, 0, 0, 0, 0])
    return Frame(height, width, sampling, tuple(tables), restart, seg_start, seg_end, blob)


# ---- files of several scans (vsc_jpeg_decode_scans_u8, csrc/jpeg_scans.hip) -------------------------------------------------------
# one table set of that entry: uint16 quant[4][64] as above, uint8 bits[8][16] and uint8 vals[8][256] of the Huffman tables DC0 .. DC3,
# AC0 .. AC3, one byte of quantisation tables present, one of Huffman tables present (bit = 4 * class + id) and six bytes of zero
SCAN_TABLE_SET_BYTES = 512 + 128 + 2048 + 8
SCAN_ROW = 10                                         # int64 per scan of the call's scan table


class Scan(NamedTuple):
    seg_start: int                                 # the scan's entropy-coded segment is data[seg_start:seg_end], up to the next marker
    seg_end: int
    comps: Tuple[int, ...]                         # the components in the scan, as indices into the frame's, ascending
    huff: Tuple[Tuple[int, int], ...]              # per component of the scan: (DC Huffman table, AC Huffman table)
    ss: int
    se: int
    ah: int
    al: int
    restart: int                                   # MCUs of the scan's own geometry per restart interval at this scan, 0: none
    tables: bytes                                  # SCAN_TABLE_SET_BYTES: the tables in force at this scan

    @property
    def comp_mask(self) -> int:
        return sum(1 << c for c in self.comps)

    @property
    def huff_word(self) -> int:
        """byte c (c: the component's index in the frame) = DC table | AC table << 2"""
        return sum((td | ta << 2) << (8 * c) for c, (td, ta) in zip(self.comps, self.huff))


class ScanFrame(NamedTuple):
    height: int
    width: int
    sampling: int
    quant: Tuple[int, ...]                         # per component: its quantisation table, in the first scan's table set
    progressive: bool                              # SOF2
    scans: Tuple[Scan, ...]                        # in file order; together they bring every coefficient of every component to Al = 0

    @property
    def comp_word(self) -> int:
        return sum(tq << (8 * c) for c, tq in enumerate(self.quant))


SCAN_REASONS = ("scan_script", "incomplete_scans", "truncated_scans", "quant_redefined")
REASONS = REASONS + SCAN_REASONS
_SCANS_TAKE = ("progressive", "multiple_scans", "huffman_table_id")     # what parse refuses and parse_scans looks at again


def widen_tables(blob: bytes) -> bytes:
    """a table set of TABLE_SET_BYTES -> the same tables as one of SCAN_TABLE_SET_BYTES"""
    b = np.frombuffer(blob, dtype=np.uint8)
    bits, vals = np.zeros((8, 16), np.uint8), np.zeros((8, 256), np.uint8)
    bits[[0, 1, 4, 5]] = b[512:576].reshape(4, 16)
    vals[[0, 1, 4, 5]] = b[576:1600].reshape(4, 256)
    hmask = int(b[1601])
    return b[:512].tobytes() + bits.tobytes() + vals.tobytes() + bytes([int(b[1600]), (hmask & 3) | (hmask >> 2 & 3) << 4, 0, 0, 0, 0, 0, 0])


def as_scan_frame(f: Frame) -> ScanFrame:
    """a frame of one sequential scan as the scan list vsc_jpeg_decode_scans_u8 takes"""
    n = len(f.comp_tables)
    scan = Scan(f.seg_start, f.seg_end, tuple(range(n)), tuple((td, ta) for _, td, ta in f.comp_tables), 0, 63, 0, 0, f.restart, widen_tables(f.tables))
    return ScanFrame(f.height, f.width, f.sampling, tuple(tq for tq, _, _ in f.comp_tables), False, (scan,))


def parse_scans(data) -> Union[Frame, ScanFrame, Refusal]:
    """``parse`` for the opt-in entry: the same Frame for a file parse accepts; a ScanFrame for a progressive file (SOF2), a
    sequential file of several scans and a file that uses Huffman table ids 0 .. 3; a Refusal for everything else.  The scan script
    is checked as libjpeg checks it (jdmarker, jdphuff start_pass) and a script libjpeg would warn about is refused; so is a file
    whose scans leave a coefficient unfinished or that ends before EOI: those are decoded with block smoothing or truncation handling."""
    first = parse(data)
    if isinstance(first, Frame) or first.reason not in _SCANS_TAKE:
        return first
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    n = len(a)
    quant = np.zeros((4, 64), np.uint16)
    bits = np.zeros((8, 16), np.uint8)
    vals = np.zeros((8, 256), np.uint8)
    qmask = hmask = 0
    sof = None
    progressive = False
    restart = 0
    jfif = False
    adobe = None
    scans: List[Scan] = []
    geometry = None                                   # (sampling, comps) once the first scan has checked the frame header
    state = None                                      # per component: the Al every coefficient stands at, -1: not yet coded
    pos = 2
    while True:
        if pos + 2 > n:
            return Refusal("truncated_scans" if scans else "truncated_header", "the file ends before EOI" if scans else "the file ends before its scan")
        if a[pos] != 0xFF:
            return Refusal("bad_header", f"byte {int(a[pos]):#x} at {pos} where a marker should be")
        m = int(a[pos + 1])
        if m == 0xFF:
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            pos += 2
            continue
        if m == 0xD9:
            if not scans:
                return Refusal("truncated_header", "EOI before any scan")
            break
        if pos + 4 > n:
            return Refusal("truncated_scans" if scans else "truncated_header", "the file ends inside a marker segment")
        length = int(a[pos + 2]) << 8 | int(a[pos + 3])
        if length < 2:
            return Refusal("bad_header", f"marker {m:#x} with length {length}")
        if pos + 2 + length > n:
            return Refusal("truncated_scans" if scans else "truncated_header", f"the file ends inside the segment of marker {m:#x}")
        seg = a[pos + 4:pos + 2 + length]
        if m in _SOF_REFUSED and m != 0xC2:
            return Refusal(*_SOF_REFUSED[m])
        if m == 0xCC:
            return Refusal("arithmetic", "arithmetic conditioning (DAC)")
        if m in (0xC0, 0xC1, 0xC2):
            if sof is not None:
                return Refusal("hierarchical", "a second frame header")
            if len(seg) < 6 or len(seg) < 6 + 3 * int(seg[5]):
                return Refusal("bad_header", "short SOF segment")
            progressive = m == 0xC2
            sof = (int(seg[0]), int(seg[1]) << 8 | int(seg[2]), int(seg[3]) << 8 | int(seg[4]),
                   [(int(seg[6 + 3 * c]), int(seg[7 + 3 * c]) >> 4, int(seg[7 + 3 * c]) & 15, int(seg[8 + 3 * c])) for c in range(int(seg[5]))])
        elif m == 0xDB:
            if scans:
                return Refusal("quant_redefined", "a quantisation table behind the first scan")
            at = 0
            while at < len(seg):
                pq, tq = int(seg[at]) >> 4, int(seg[at]) & 15
                if pq != 0:
                    return Refusal("quant16", "a 16-bit quantisation table")
                if tq > 3 or at + 65 > len(seg):
                    return Refusal("bad_header", "bad DQT segment")
                quant[tq] = seg[at + 1:at + 65]
                qmask |= 1 << tq
                at += 65
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                tc, th = int(seg[at]) >> 4, int(seg[at]) & 15
                if tc > 1 or th > 3 or at + 17 > len(seg):
                    return Refusal("bad_header", "bad DHT segment")
                count = int(seg[at + 1:at + 17].sum())
                if count > 256 or at + 17 + count > len(seg):
                    return Refusal("bad_header", "bad DHT segment")
                t = 4 * tc + th
                bits[t] = seg[at + 1:at + 17]
                vals[t] = 0
                vals[t, :count] = seg[at + 17:at + 17 + count]
                hmask |= 1 << t
                at += 17 + count
        elif m == 0xDD:
            if len(seg) < 2:
                return Refusal("bad_header", "short DRI segment")
            restart = int(seg[0]) << 8 | int(seg[1])
        elif m == 0xDC:
            return Refusal("bad_header", "a DNL marker")
        elif m == 0xE0:
            jfif = jfif or (len(seg) >= 5 and bytes(seg[:5]) == b"JFIF\0")
        elif m == 0xEE:
            if len(seg) >= 12 and bytes(seg[:5]) == b"Adobe":
                adobe = int(seg[11])
        elif m == 0xDA:
            if geometry is None:
                if sof is None:
                    return Refusal("bad_header", "a scan without a frame header")
                precision, height, width, comps = sof
                if precision != 8:
                    return Refusal("precision", f"{precision}-bit samples")
                if len(comps) not in (1, 3):
                    return Refusal("components", f"{len(comps)} components")
                if height < 1 or width < 1 or height > MAX_SIDE or width > MAX_SIDE:
                    return Refusal("size", f"{height} x {width} pixels (1 .. {MAX_SIDE} a side; a height of 0 is set by a DNL marker)")
                if len(comps) == 1:
                    sampling = GRAY
                else:
                    if adobe is not None and adobe == 0:
                        return Refusal("adobe_rgb", "Adobe APP14 transform 0: the three components are RGB")
                    if adobe is None and not jfif and tuple(c[0] for c in comps) == (82, 71, 66):
                        return Refusal("rgb_component_ids", "components named R, G, B without a JFIF or Adobe marker")
                    fac = tuple((c[1], c[2]) for c in comps)
                    if fac[1:] != ((1, 1), (1, 1)) or fac[0] not in ((1, 1), (2, 1), (2, 2)):
                        return Refusal("sampling", f"sampling factors {fac}")
                    sampling = {(1, 1): S444, (2, 1): S422, (2, 2): S420}[fac[0]]
                for c, comp in enumerate(comps):
                    if comp[3] > 3 or not (qmask >> comp[3] & 1):
                        return Refusal("missing_tables", f"component {c} uses a quantisation table the file does not define")
                if len(set(c[0] for c in comps)) != len(comps):
                    return Refusal("bad_header", "two components of one name")
                geometry = (sampling, comps)
                state = np.full((len(comps), 64), -1, np.int32)
            sampling, comps = geometry
            ns = int(seg[0]) if len(seg) else 0
            if ns < 1 or ns > len(comps) or len(seg) < 1 + 2 * ns + 3:
                return Refusal("bad_header", "bad SOS segment")
            ss, se, ahal = (int(v) for v in seg[1 + 2 * ns:4 + 2 * ns])
            ah, al = ahal >> 4, ahal & 15
            ids = [c[0] for c in comps]
            which, huff = [], []
            for c in range(ns):
                cs, tdta = int(seg[1 + 2 * c]), int(seg[2 + 2 * c])
                if cs not in ids or (which and ids.index(cs) <= which[-1]):
                    return Refusal("bad_header", "the scan lists the components in another order than the frame")
                which.append(ids.index(cs))
                huff.append((tdta >> 4, tdta & 15))
            if progressive:
                if ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and ns != 1) or al > 13 or (ah != 0 and al != ah - 1):
                    return Refusal("scan_script", f"a scan of coefficients {ss} .. {se}, approximation {ahal:#x}, of {ns} components")
            elif (ss, se, ahal) != (0, 63, 0):
                return Refusal("scan_script", f"a sequential scan of coefficients {ss} .. {se}, approximation {ahal:#x}")
            for c, (td, ta) in zip(which, huff):
                need_dc, need_ac = ss == 0 and ah == 0, se > 0
                if td > 3 or ta > 3 or (need_dc and not (hmask >> td & 1)) or (need_ac and not (hmask >> (4 + ta) & 1)):
                    return Refusal("missing_tables", f"component {c} uses a Huffman table the file does not define")
                if ss > 0 and state[c, 0] < 0:
                    return Refusal("scan_script", f"an AC scan of component {c} before its first DC scan")
                band = state[c, ss:se + 1]
                if not (band == (ah if ah else -1)).all():
                    return Refusal("scan_script", f"component {c}, coefficients {ss} .. {se}: successive approximation {ah} does not continue {band.tolist()}")
                state[c, ss:se + 1] = al
            seg_start = pos + 2 + length
            seg_end, marker = scan_end(a, seg_start)
            if marker == -1:
                return Refusal("truncated_scans", f"the file ends inside scan {len(scans) + 1}")
            blob = quant.astype("<u2").tobytes() + bits.tobytes() + vals.tobytes() + bytes([qmask, hmask, 0, 0, 0, 0, 0, 0])
            scans.append(Scan(seg_start, seg_end, tuple(which), tuple(huff), ss, se, ah, al, restart, blob))
            pos = seg_end
            continue
        pos += 2 + length
    if (state != 0).any():
        return Refusal("incomplete_scans", "the scans leave " + ("coefficients at a successive approximation above 0" if (state > 0).any() else "coefficients uncoded"))
    sampling, comps = geometry
    return ScanFrame(sof[1], sof[2], sampling, tuple(c[3] for c in comps), progressive, tuple(scans))


def scan_rows(frames: Sequence[Union[Frame, ScanFrame]], file_offsets: Sequence[int], out_offsets: Sequence[int],
              sets: "ScanTableSets") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """the tables of one vsc_jpeg_decode_scans_u8 call: (frame table int64 [n, FRAME_ROW], scan table int64 [scans, SCAN_ROW],
    int64 ptr [n + 1]: frame i's scans are rows ptr[i] .. ptr[i + 1]).  A frame row = (0, 0, height, width, sampling class, 0, the
    table set of the quantisation tables, output byte offset, component word: byte c = quantisation table of component c, 0); a scan
    row = (segment offset, segment length, component mask, Ss, Se, Ah, Al, restart interval, table set, Huffman word)."""
    frames = [as_scan_frame(f) if isinstance(f, Frame) else f for f in frames]
    rows = np.zeros((len(frames), FRAME_ROW), np.int64)
    ptr = np.zeros(len(frames) + 1, np.int64)
    srows = []
    for i, (f, at, out) in enumerate(zip(frames, file_offsets, out_offsets)):
        rows[i] = (0, 0, f.height, f.width, f.sampling, 0, sets.add(f.scans[0].tables), out, f.comp_word, 0)
        for s in f.scans:
            srows.append((at + s.seg_start, s.seg_end - s.seg_start, s.comp_mask, s.ss, s.se, s.ah, s.al, s.restart, sets.add(s.tables), s.huff_word))
        ptr[i + 1] = len(srows)
    return rows, np.asarray(srows, np.int64).reshape(len(srows), SCAN_ROW), ptr


def pack_scans(files: Sequence) -> Tuple[np.ndarray, np.ndarray, List[Union[Frame, ScanFrame, Refusal]]]:
    """``pack`` with parse_scans"""
    arrays = [np.frombuffer(f, dtype=np.uint8) for f in files]
    offsets = np.zeros(len(arrays) + 1, np.int64)
    np.cumsum([len(x) for x in arrays], out=offsets[1:])
    data = np.concatenate(arrays) if arrays else np.zeros(0, np.uint8)
    return data, offsets, [parse_scans(x) for x in arrays]


class TableSets:
    """table sets of a call, de-duplicated by content"""

    def __init__(self):
        self.index = {}
        self.blobs: List[bytes] = []

    def add(self, blob: bytes) -> int:
        i = self.index.get(blob)
        if i is None:
            assert len(blob) == TABLE_SET_BYTES
            i = self.index[blob] = len(self.blobs)
            self.blobs.append(blob)
        return i

    def __len__(self):
        return len(self.blobs)

    def array(self) -> np.ndarray:
        """uint8 [n_table_sets, TABLE_SET_BYTES]"""
        return np.frombuffer(b"".join(self.blobs), dtype=np.uint8).reshape(len(self.blobs), TABLE_SET_BYTES).copy()


class ScanTableSets(TableSets):
    """table sets of a vsc_jpeg_decode_scans_u8 call"""
    nbytes = SCAN_TABLE_SET_BYTES

    def add(self, blob: bytes) -> int:
        i = self.index.get(blob)
        if i is None:
            assert len(blob) == SCAN_TABLE_SET_BYTES
            i = self.index[blob] = len(self.blobs)
            self.blobs.append(blob)
        return i

    def array(self) -> np.ndarray:
        return np.frombuffer(b"".join(self.blobs), dtype=np.uint8).reshape(len(self.blobs), SCAN_TABLE_SET_BYTES).copy()


def frame_rows(frames: Sequence[Frame], file_offsets: Sequence[int], out_offsets: Sequence[int], sets: TableSets) -> np.ndarray:
    """the frame table of one call, int64 [n, FRAME_ROW]: (segment offset, segment length, height, width, sampling class, restart
    interval, table set, output byte offset, component word, 0); ``file_offsets[i]`` is where file i starts in the call's bytes"""
    rows = np.zeros((len(frames), FRAME_ROW), np.int64)
    for i, (f, at, out) in enumerate(zip(frames, file_offsets, out_offsets)):
        rows[i] = (at + f.seg_start, f.seg_end - f.seg_start, f.height, f.width, f.sampling, f.restart, sets.add(f.tables), out, f.comp_word, 0)
    return rows


def pack(files: Sequence) -> Tuple[np.ndarray, np.ndarray, List[Union[Frame, Refusal]]]:
    """The files of one video (bytes each) -> (uint8 concatenation, int64 offsets [n + 1], [Frame or Refusal per file])"""
    arrays = [np.frombuffer(f, dtype=np.uint8) for f in files]
    offsets = np.zeros(len(arrays) + 1, np.int64)
    np.cumsum([len(x) for x in arrays], out=offsets[1:])
    data = np.concatenate(arrays) if arrays else np.zeros(0, np.uint8)
    return data, offsets, [parse(x) for x in arrays]


# ---- cutting a frame into items (vsc_jpeg_decode_split_u8, csrc/jpeg_split.hip) ----------------------------------------------------
SPLITS = ("none", "markers", "substreams", "all")    # --decode_split; the entry's mode is the index: bit 1 markers, bit 2 sub-streams
SPLIT_SUB_BYTES, SPLIT_ROUNDS, SPLIT_ITEM_BYTES = 1024, 2, 1024


def mcus(frame: Frame) -> int:
    mcu_h, mcu_w = MCU_SIDE[frame.sampling]
    return -(-frame.height // mcu_h) * -(-frame.width // mcu_w)


def restart_offsets(data, frame: Frame) -> np.ndarray:
    """int32 offsets, from the start of the frame's entropy-coded segment, of every FF D0..D7 in it, ascending"""
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    seg = a[frame.seg_start:frame.seg_end]
    if len(seg) < 2:
        return np.zeros(0, np.int32)
    return np.flatnonzero((seg[:-1] == 0xFF) & (seg[1:] >= 0xD0) & (seg[1:] <= 0xD7)).astype(np.int32)


def expected_restarts(frame: Frame) -> int:
    """how many RSTn a frame with a restart interval holds; -1 for a frame without one.  Only a frame whose marker scan finds
    exactly this many is cut at its markers"""
    return -(-mcus(frame) // frame.restart) - 1 if frame.restart else -1


def restart_rows(files: Sequence, records: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """the CSR of marker offsets of one call or video: (int64 ptr [n + 1], int32 off); a Refusal or a frame without restart
    interval has an empty row"""
    rows = [restart_offsets(np.frombuffer(f, dtype=np.uint8), r) if isinstance(r, Frame) and r.restart else np.zeros(0, np.int32)
            for f, r in zip(files, records)]
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    return ptr, (np.concatenate(rows) if rows else np.zeros(0, np.int32)).astype(np.int32)


def concat_restart_rows(parts: Sequence[Tuple[np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, np.ndarray]:
    """the CSRs of several videos -> the CSR of the call that decodes them together"""
    ptr, at = [np.zeros(1, np.int64)], 0
    for p, _ in parts:
        ptr.append(p[1:] + at)
        at += int(p[-1])
    off = [o for _, o in parts if len(o)]
    return np.concatenate(ptr), (np.concatenate(off) if off else np.zeros(0, np.int32)).astype(np.int32)
