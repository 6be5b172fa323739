"""The executable contract of vsc_jpeg_decode_scans_u8 (csrc/jpeg_scans.hip): a numpy-only decoder of JPEG files of several scans --
progressive (SOF2), sequential in several scans, Huffman table ids 0 .. 3 -- whose output is
``np.asarray(Image.open(f).convert("RGB"))`` bit for bit.  Only the entropy stage is stated here: the scans of a complete file
accumulate the quantised coefficients its sequential twin holds, and everything behind them (dequantisation, jpeg_idct_islow,
fancy upsampling, colour) is tests/jpeg_decode_contract.py, unchanged.  libjpeg smooths blocks only while a coefficient's precision
is still unknown, which vsc_hip.jpeg.parse_scans excludes (incomplete_scans).

Coefficient accumulation (ITU T.81 G.1 - G.2, libjpeg's jdphuff.c), per scan (Ss, Se, Ah, Al):

  * DC first (Ss = 0, Ah = 0): the difference is added to the component's predictor; the coefficient is predictor << Al.
  * DC refine (Ss = 0, Ah > 0): one bit per block, ORed in at 1 << Al.  No Huffman code is read.
  * AC first: symbols (run r, size s).  s > 0: r coefficients are skipped, the value of s bits is stored << Al.  s = 0, r = 15: 16
    coefficients are skipped.  s = 0, r < 15: EOBRUN = (1 << r) + r more bits; this block and the EOBRUN - 1 that follow are done.
  * AC refine: s is 0 or 1.  s = 1: one sign bit FIRST, then the walk: from the current coefficient on, every coefficient that is
    already non-zero takes one correction bit (1: 1 << Al is added away from zero), every zero one counts down r; the new
    coefficient, +-(1 << Al), lands on the (r + 1)-th ZERO coefficient.  s = 0, r = 15: the same walk over 16 zeros, nothing is
    placed.  s = 0, r < 15: EOBRUN as above, and the rest of this block's band and the whole band of each of the EOBRUN - 1 blocks that
    follow still take one correction bit per non-zero coefficient.
  * a sequential scan (Ss = 0, Se = 63): tests/jpeg_decode_contract.py's block.

Geometry: a scan of one component walks that component's own blocks, ceil(component width / 8) x ceil(component height / 8),
row-major, NOT the MCU-padded grid; a scan of several components walks the frame's MCUs.  The restart interval in force at the scan
counts these units; a restart byte-aligns, wants RSTn in sequence, and resets the DC predictors and EOBRUN.

Faults (the frame's status, VSC_JPEG_STATUS_*; the frame stops at the first): DATA 1 a block read bits behind the end of its
segment or interval; CODE 2 no code of the table starts the next bits, a DC size above 16, or an AC-refine size above 1; RUN 3 a
run past the end of the band (past the last zero coefficient in a refine scan), or an EOBRUN longer than the blocks left in its
restart interval or scan (libjpeg would drop the excess silently: such a file is damaged); RESTART 4 a missing or wrong RSTn;
SCRIPT 5 a scan the host check should have excluded.  Values wrap to 16 bits as libjpeg's JCOEF does."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_decode_contract as base  # noqa: E402
from jpeg_decode_contract import jpeg  # noqa: E402

DATA, CODE, RUN, RESTART, SCRIPT = 1, 2, 3, 4, 5


class Fault(Exception):
    def __init__(self, status):
        self.status = status


def w16(v):
    return ((v + 32768) & 65535) - 32768


class Bits:
    """the bit reader of csrc/jpeg_decode_dev.h: zeros behind a marker or the end; avail < 0 once more bits were taken than existed"""

    def __init__(self, seg):
        self.seg = bytes(seg)
        self.start(0)

    def start(self, byte):
        self.pos, self.acc, self.nb, self.avail, self.stop = byte, 0, 0, 0, False

    def fill(self):
        seg = self.seg
        while self.nb <= 48:
            v = 0
            if not self.stop:
                if self.pos >= len(seg):
                    self.stop = True
                else:
                    v = seg[self.pos]
                    if v != 0xFF:
                        self.pos += 1
                    elif self.pos + 1 < len(seg) and seg[self.pos + 1] == 0:
                        self.pos += 2
                    else:
                        self.stop, v = True, 0
                if not self.stop:
                    self.avail += 8
            self.acc = self.acc << 8 | v
            self.nb += 8

    def peek16(self):
        self.fill()
        return (self.acc >> (self.nb - 16)) & 0xFFFF

    def skip(self, n):
        self.nb -= n
        self.avail -= n
        self.acc &= (1 << self.nb) - 1

    def get(self, n):
        if n == 0:
            return 0
        self.fill()
        x = (self.acc >> (self.nb - n)) & ((1 << n) - 1)
        self.skip(n)
        return x

    def receive(self, s):
        x = self.get(s)
        return x if x >> (s - 1) else x - (1 << s) + 1

    def symbol(self, lut):
        e = lut[self.peek16()]
        if not e:
            raise Fault(CODE)
        self.skip(e >> 8)
        return e & 255

    def restart(self, number):
        self.fill()
        seg = self.seg
        if not (self.stop and self.avail < 8 and self.pos + 2 <= len(seg) and seg[self.pos] == 0xFF and seg[self.pos + 1] == 0xD0 + number):
            raise Fault(RESTART)
        self.start(self.pos + 2)


def scan_tables(blob):
    """a table set of SCAN_TABLE_SET_BYTES -> (quant [4][64] zigzag, 8 lookup tables: DC0 .. DC3, AC0 .. AC3)"""
    b = np.frombuffer(blob, dtype=np.uint8)
    quant = b[:512].view("<u2").reshape(4, 64).astype(np.int64)
    bits, vals = b[512:640].reshape(8, 16), b[640:2688].reshape(8, 256)
    present = int(b[2689])
    return quant, [base.huffman_lut(bits[t], vals[t]) if present >> t & 1 else None for t in range(8)]


def geometry(frame):
    """-> (hs, vs, mx, my, per component: (blocks per MCU along x, along y, own block columns, own block rows))"""
    mcu_h, mcu_w = jpeg.MCU_SIDE[frame.sampling]
    hs, vs = mcu_w // 8, mcu_h // 8
    my, mx = -(-frame.height // mcu_h), -(-frame.width // mcu_w)
    comps = [(hs, vs, -(-frame.width // 8), -(-frame.height // 8))]
    cw, ch = -(-frame.width // hs), -(-frame.height // vs)
    comps += [(1, 1, -(-cw // 8), -(-ch // 8))] * (len(frame.quant) - 1)
    return hs, vs, mx, my, comps


ZZ = jpeg.ZIGZAG.tolist()


def block_sequential(b, out, dc, ac, pred):
    s = b.symbol(dc)
    if s > 16:
        raise Fault(CODE)
    if s:
        pred = w16(pred + b.receive(s))
    out[0] = pred
    k = 1
    while k < 64:
        s = b.symbol(ac)
        r, s = s >> 4, s & 15
        if s:
            k += r
            if k > 63:
                raise Fault(RUN)
            out[ZZ[k]] = b.receive(s)
            k += 1
        elif r == 15:
            k += 16
        else:
            break
    return pred


def eobrun_of(b, r, left):
    run = (1 << r) + b.get(r)
    if run > left:
        raise Fault(RUN)
    return run


def block_ac_first(b, out, ac, ss, se, al, left):
    """-> the EOBRUN that starts with this block (0: none)"""
    k = ss
    while k <= se:
        s = b.symbol(ac)
        r, s = s >> 4, s & 15
        if s:
            k += r
            if k > se:
                raise Fault(RUN)
            out[ZZ[k]] = w16(b.receive(s) << al)
            k += 1
        elif r == 15:
            k += 16
        else:
            return eobrun_of(b, r, left)
    return 0


def correct(b, out, ks, al):
    """one correction bit for each of the (non-zero) coefficients ks, in order"""
    p1 = 1 << al
    for k in ks:
        if b.get(1):
            v = int(out[ZZ[k]])
            if not v & p1:
                out[ZZ[k]] = w16(v + p1 if v >= 0 else v - p1)


def block_ac_refine(b, out, ac, ss, se, al, left, eobrun):
    """-> the EOBRUN in force behind this block's symbols (this block included; the caller counts it down)"""
    k = ss
    if eobrun == 0:
        while k <= se:
            s = b.symbol(ac)
            r, s = s >> 4, s & 15
            if s > 1:
                raise Fault(CODE)
            if s == 0 and r < 15:
                eobrun = eobrun_of(b, r, left)
                break
            new = 0
            if s:
                new = (1 << al) if b.get(1) else -(1 << al)
            passed, at = [], -1
            for j in range(k, se + 1):
                if out[ZZ[j]] != 0:
                    passed.append(j)
                else:
                    r -= 1
                    if r < 0:
                        at = j
                        break
            if at < 0:
                raise Fault(RUN)
            correct(b, out, passed, al)
            if s:
                out[ZZ[at]] = new
            k = at + 1
    if eobrun > 0:
        correct(b, out, [j for j in range(k, se + 1) if out[ZZ[j]] != 0], al)
    return eobrun


def coefficients(frame, data):
    """a ScanFrame and its file -> (per component int64 [block rows, block columns, 64] natural order, MCU-padded; status)"""
    hs, vs, mx, my, comps = geometry(frame)
    coef = [np.zeros((my * v, mx * h, 64), np.int64) for h, v, _, _ in comps]
    try:
        for scan in frame.scans:
            _, luts = scan_tables(scan.tables)
            b = Bits(data[scan.seg_start:scan.seg_end])
            seq, dc_scan = (scan.ss, scan.se) == (0, 63), scan.se == 0
            if not seq and not dc_scan and len(scan.comps) != 1:
                raise Fault(SCRIPT)
            if len(scan.comps) == 1:
                _, _, bw, bh = comps[scan.comps[0]]
                units, per_row = bw * bh, bw
            else:
                units, per_row = mx * my, mx
            pred = [0] * len(comps)
            eobrun = 0
            for u in range(units):
                if scan.restart and u and u % scan.restart == 0:
                    b.restart((u // scan.restart - 1) & 7)
                    pred = [0] * len(comps)
                    eobrun = 0
                left = min(units, (u // scan.restart + 1) * scan.restart) - u if scan.restart else units - u
                row, col = divmod(u, per_row)
                for c, (td, ta) in zip(scan.comps, scan.huff):
                    h, v = (1, 1) if len(scan.comps) == 1 else comps[c][:2]
                    for blk in range(h * v):
                        out = coef[c][row * v + blk // h, col * h + blk % h]
                        if seq:
                            pred[c] = block_sequential(b, out, luts[td], luts[4 + ta], pred[c])
                        elif dc_scan and scan.ah == 0:
                            s = b.symbol(luts[td])
                            if s > 16:
                                raise Fault(CODE)
                            if s:
                                pred[c] = w16(pred[c] + b.receive(s))
                            out[0] = w16(pred[c] << scan.al)
                        elif dc_scan:
                            if b.get(1):
                                out[0] = w16(int(out[0]) | 1 << scan.al)
                        elif scan.ah == 0:
                            if eobrun == 0:
                                eobrun = block_ac_first(b, out, luts[4 + ta], scan.ss, scan.se, scan.al, left)
                            if eobrun:
                                eobrun -= 1
                        else:
                            eobrun = block_ac_refine(b, out, luts[4 + ta], scan.ss, scan.se, scan.al, left, eobrun)
                            if eobrun:
                                eobrun -= 1
                        if b.avail < 0:
                            raise Fault(DATA)
    except Fault as f:
        return coef, f.status
    return coef, 0


def decode_frame(frame, data):
    """-> (uint8 [H, W, 3] or None for a frame that stopped, status)"""
    if isinstance(frame, jpeg.Frame):
        frame = jpeg.as_scan_frame(frame)
    coef, status = coefficients(frame, bytes(data))
    if status:
        return None, status
    h, w = frame.height, frame.width
    quant, _ = scan_tables(frame.scans[0].tables)
    planes = [base.plane(c, quant[tq]) for c, tq in zip(coef, frame.quant)]
    y = planes[0][:h, :w]
    if frame.sampling == jpeg.GRAY:
        return np.repeat(y[:, :, None], 3, axis=2), 0
    if frame.sampling == jpeg.S444:
        cb, cr = planes[1][:h, :w], planes[2][:h, :w]
    elif frame.sampling == jpeg.S422:
        cb, cr = (base.upsample_h2v1(p[:h], -(-w // 2), w) for p in planes[1:])
    else:
        cb, cr = (base.upsample_h2v2(p, -(-h // 2), -(-w // 2), h, w) for p in planes[1:])
    return base.ycc_to_rgb(y, cb, cr), 0


def decode(data):
    """the bytes of one file that parse_scans accepts -> uint8 [H, W, 3]"""
    frame = jpeg.parse_scans(data)
    assert isinstance(frame, (jpeg.Frame, jpeg.ScanFrame)), frame
    out, status = decode_frame(frame, data)
    assert status == 0, status
    return out
