"""The executable contract of vsc_jpeg_decode_split_u8 (csrc/jpeg_split.hip), numpy only, on top of jpeg_decode_contract.py and
vsc_hip.jpeg: how a frame is cut into ITEMS -- runs of consecutive blocks with a known start state (byte and bit in the segment,
first block in scan order, number of blocks, DC predictors) -- and that decoding the items gives jpeg_decode_contract.decode's
bytes.

  * restart markers: ``jpeg.restart_offsets`` finds every FF D0..D7 of the segment; the frame is cut only if their number is
    ceil(MCUs / Ri) - 1.  Consecutive intervals are grouped until an item holds at least ``item_bytes`` entropy bytes.
  * sub-streams (frames without restart interval): the segment is cut every ``sub_bytes`` raw bytes.  A state is (raw bit position
    of a block start, slot of the block in its MCU).  ``run`` decodes symbols only from a state to the first block start at or
    behind the sub-stream's end (or the segment's), moving the block start ONE BIT ON when a code is in no table, a run passes
    coefficient 63 or the bytes run out.  Round 0 starts sub-stream i at (8 i sub_bytes, 0); each verification round starts it
    at sub-stream i - 1's exit of the round before.  The frame has converged iff the last round changed no exit; it keeps its cut
    iff it has, the block counts add up to the frame's and every start slot fits.  Otherwise: one item, the whole frame.

Raw positions count the bytes of the segment as they stand, FF 00 pairs as two; a reader that starts at a byte takes it as data
whatever stands in front of it.  ``split(data, ...)`` returns a ``Split``; ``stats`` adds the four numbers of
vsc_jpeg_decode_stats over the frames of a call; ``decode(data, items)`` decodes item by item."""
import os
import sys
from typing import NamedTuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_decode_contract as base  # noqa: E402
from vsc_hip import jpeg  # noqa: E402


class Item(NamedTuple):
    byte: int
    bit: int
    block0: int
    nblocks: int
    end_off: int       # where the RSTn behind the item stands in the segment, -1: the frame's last item or no marker
    pred: tuple


class Split(NamedTuple):
    kind: str          # "markers", "substreams", "fallback" (the mode wanted a cut, the frame is one item) or "none"
    items: tuple       # of Item; empty items included
    exits: tuple       # per round (0: speculative): ((raw bit position, slot) per sub-stream); () unless sub-streams were run
    converged: bool
    right_after_round0: int


def wrap16(v):
    """an int16 as the device holds it"""
    return ((v + 0x8000) & 0xFFFF) - 0x8000


def geometry(frame):
    """-> (blocks per MCU, component of every slot, MCUs)"""
    mcu_h, mcu_w = jpeg.MCU_SIDE[frame.sampling]
    slots = [0] * ((mcu_h // 8) * (mcu_w // 8)) + list(range(1, len(frame.comp_tables)))
    return len(slots), slots, jpeg.mcus(frame)


class Stream:
    """the data bytes of a segment from raw byte ``start`` up to the first marker or the end: 16-bit windows at every bit, and
    the raw byte at which every data byte stands"""

    def __init__(self, seg, start):
        raw, at, n = [], start, len(seg)
        data = bytearray()
        while at < n:
            v = seg[at]
            if v != 0xFF:
                raw.append(at)
                at += 1
            elif at + 1 < n and seg[at + 1] == 0:
                raw.append(at)
                at += 2
            else:
                break
            data.append(v)
        self.raw = raw + [at]                       # raw[len]: where the reader stops
        self.index = {r: k for k, r in enumerate(raw)}
        self.nbits = 8 * len(data)
        bits = np.concatenate([np.unpackbits(np.frombuffer(bytes(data), np.uint8)), np.zeros(48, np.uint8)]).astype(np.int32)
        w = np.zeros(len(bits) - 16, np.int32)
        for k in range(16):
            w += bits[k:k + len(w)] << (15 - k)
        self.w = w.tolist()

    def rawpos(self, pos):
        return 8 * self.raw[pos >> 3] + (pos & 7)


class Reader:
    """streams of one segment by start byte: the one from byte 0 serves every start at one of its data bytes"""

    def __init__(self, seg):
        self.seg = bytes(seg)
        self.main = Stream(self.seg, 0)
        self.others = {}

    def at(self, rawbit):
        """-> (stream, its bit position) of a reader started at raw bit position ``rawbit``"""
        byte, bit = rawbit >> 3, rawbit & 7
        k = self.main.index.get(byte)
        if k is not None:
            return self.main, 8 * k + bit
        if byte not in self.others:
            self.others[byte] = Stream(self.seg, byte)
        return self.others[byte], bit


def skip_block(s, pos, dc, ac):
    """the symbols of one block from bit ``pos`` of stream s -> (position behind it, DC difference), or None where the device
    moves one bit on"""
    w, nbits = s.w, s.nbits
    if pos >= nbits:
        return None
    e = dc[w[pos]]
    if not e or (e & 255) > 16:
        return None
    pos += e >> 8
    n = e & 255
    diff = 0
    if n:
        if pos >= nbits:
            return None
        x = w[pos] >> (16 - n)
        pos += n
        diff = x if x >> (n - 1) else x - (1 << n) + 1
    k = 1
    while k < 64:
        if pos >= nbits:
            return None
        e = ac[w[pos]]
        if not e:
            return None
        pos += e >> 8
        r, n = (e & 255) >> 4, e & 15
        if n:
            k += r
            if k > 63:
                return None
            pos += n
            k += 1
        elif r == 15:
            k += 16
        else:
            break
    return (pos, diff) if pos <= nbits else None


def substreams(frame, seg, sub_bytes, rounds):
    """-> (exits per round, rows of the last round [(start, exit, count, sums)], changed flags of the last round)"""
    _, huff = base.tables_of(frame.tables)
    luts = [base.huffman_lut(*h) for h in huff]
    bpm, slots, _ = geometry(frame)
    reader = Reader(seg)
    nsub = -(-len(seg) // sub_bytes)
    memo = {}

    def run(i, state):
        if (i, state) in memo:
            return memo[i, state]
        pos, slot = state
        end = min(8 * sub_bytes * (i + 1), 8 * len(seg))
        count, sums = 0, [0, 0, 0]
        s = at = None
        while pos < end:
            if s is None:
                s, at = reader.at(pos)
            c = slots[slot]
            _, td, ta = frame.comp_tables[c]
            got = skip_block(s, at, luts[td], luts[2 + ta])
            if got is None:
                pos, s = pos + 1, None
            else:
                at = got[0]
                pos = s.rawpos(at)
                sums[c] = (sums[c] + got[1]) & 0xFFFF
                count += 1
                slot = (slot + 1) % bpm
        memo[i, state] = ((pos, slot), count, tuple(sums))
        return memo[i, state]

    starts = [(0, 0)] + [(8 * sub_bytes * i, 0) for i in range(1, nsub)]
    rows = [run(i, starts[i]) for i in range(nsub)]
    exits = [tuple(r[0] for r in rows)]
    changed = [False] + [True] * (nsub - 1)
    for _ in range(rounds):
        new_starts = [(0, 0)] + [rows[i - 1][0] for i in range(1, nsub)]
        new_rows = [run(i, new_starts[i]) for i in range(nsub)]
        changed = [a[0] != b[0] for a, b in zip(new_rows, rows)]
        starts, rows = new_starts, new_rows
        exits.append(tuple(r[0] for r in rows))
    return tuple(exits), [(starts[i],) + rows[i] for i in range(nsub)], changed


def true_exits(frame, seg, sub_bytes):
    """the exits after as many rounds as there are sub-streams: the fixed point"""
    nsub = -(-len(seg) // sub_bytes)
    return substreams(frame, seg, sub_bytes, nsub)[0][-1]


def split(data, sub_bytes=jpeg.SPLIT_SUB_BYTES, rounds=jpeg.SPLIT_ROUNDS, item_bytes=jpeg.SPLIT_ITEM_BYTES, mode=3, restarts=None):
    """how vsc_jpeg_decode_split_u8 cuts the frame of one file; ``restarts``: the marker offsets the entry is given (default: the
    parser's marker scan)"""
    frame = jpeg.parse(data)
    assert isinstance(frame, jpeg.Frame), frame
    seg = bytes(data)[frame.seg_start:frame.seg_end]
    bpm, _, mcus = geometry(frame)
    whole = (Item(0, 0, 0, mcus * bpm, -1, (0, 0, 0)),)
    if frame.restart and mode & 1:
        off = jpeg.restart_offsets(np.frombuffer(bytes(data), np.uint8), frame).tolist() if restarts is None else list(restarts)
        if len(off) != jpeg.expected_restarts(frame):
            return Split("fallback", whole, (), False, 0)
        items, first, acc, last = [], 0, 0, len(off)
        for k in range(last + 1):
            acc += (off[k] if k < last else len(seg)) - (off[k - 1] + 2 if k else 0)
            if acc < item_bytes and k < last:
                continue
            block0 = first * frame.restart * bpm
            items.append(Item(off[first - 1] + 2 if first else 0, 0, block0, min((k + 1) * frame.restart, mcus) * bpm - block0, off[k] if k < last else -1, (0, 0, 0)))
            first, acc = k + 1, 0
        return Split("markers", tuple(items), (), False, 0)
    if not frame.restart and mode & 2 and len(seg):
        exits, rows, changed = substreams(frame, seg, sub_bytes, rounds)
        right = sum(a == b for a, b in zip(exits[0], true_exits(frame, seg, sub_bytes)))
        converged = not any(changed)
        ok, blocks = converged, 0
        for i, (start, _, count, _) in enumerate(rows):
            ok = ok and start[1] == blocks % bpm
            blocks += count
        ok = ok and blocks == mcus * bpm
        if not ok:
            return Split("fallback", whole + (Item(0, 0, 0, 0, -1, (0, 0, 0)),) * (len(rows) - 1), exits, converged, right)
        items, blocks, sums = [], 0, [0, 0, 0]
        for start, _, count, s in rows:
            items.append(Item(start[0] >> 3, start[0] & 7, blocks, count, -1, tuple(wrap16(v) for v in sums)))
            blocks += count
            sums = [(a + b) & 0xFFFF for a, b in zip(sums, s)]
        return Split("substreams", tuple(items), exits, converged, right)
    wanted = (frame.restart and mode & 1) or (not frame.restart and mode & 2)
    return Split("fallback" if wanted else "none", whole, (), False, 0)


def stats(splits):
    """vsc_jpeg_decode_stats of a call whose frames were cut as ``splits``: (cut at markers, cut into sub-streams, wanted cut but
    one item, items launched)"""
    kinds = [s.kind for s in splits]
    return (kinds.count("markers"), kinds.count("substreams"), kinds.count("fallback"), sum(len(s.items) for s in splits))


def coefficients(frame, data, items):
    """jpeg_decode_contract.coefficients, item by item: every item starts a reader of its own at its (byte, bit)"""
    _, huff = base.tables_of(frame.tables)
    luts = [base.huffman_lut(*h) for h in huff]
    mcu_h, mcu_w = jpeg.MCU_SIDE[frame.sampling]
    my, mx = -(-frame.height // mcu_h), -(-frame.width // mcu_w)
    hs, vs = mcu_w // 8, mcu_h // 8
    bpm, slots, mcus = geometry(frame)
    shape = [(hs, vs)] + [(1, 1)] * (len(frame.comp_tables) - 1)
    coef = [np.zeros((my * v, mx * h, 64), np.int64) for h, v in shape]
    written = [np.zeros((my * v, mx * h), bool) for h, v in shape]
    zz = jpeg.ZIGZAG.tolist()
    seg = bytes(data)[frame.seg_start:frame.seg_end]
    reader = Reader(seg)

    def marker_ahead(s, pos, mcu):
        assert -(-pos // 8) * 8 == s.nbits, "the interval does not end at the marker"
        stop = s.raw[-1]
        assert seg[stop:stop + 2] == bytes([0xFF, 0xD0 + (mcu // frame.restart - 1) % 8]), "RSTn out of sequence"
        return stop

    for it in items:
        if it.nblocks <= 0:
            continue
        s, pos = reader.at(8 * it.byte + it.bit)
        pred = list(it.pred)
        for j in range(it.block0, it.block0 + it.nblocks):
            assert j < mcus * bpm
            mcu, slot = divmod(j, bpm)
            if frame.restart and slot == 0 and j > it.block0 and mcu % frame.restart == 0:
                s, pos = reader.at(8 * (marker_ahead(s, pos, mcu) + 2))
                pred = [0, 0, 0]
            c = slots[slot]
            _, td, ta = frame.comp_tables[c]
            dc, ac = luts[td], luts[2 + ta]
            h, v = shape[c]
            row, col = divmod(mcu, mx)
            by, bx = (row * v + slot // h, col * h + slot % h) if c == 0 else (row, col)
            assert not written[c][by, bx], "a block decoded twice"
            written[c][by, bx] = True
            out = coef[c][by, bx]
            w = s.w
            e = dc[w[pos]]
            assert e, "no such DC code"
            pos += e >> 8
            n = e & 255
            if n:
                x = w[pos] >> (16 - n)
                pos += n
                pred[c] = wrap16(pred[c] + (x if x >> (n - 1) else x - (1 << n) + 1))
            out[0] = pred[c]
            k = 1
            while k < 64:
                e = ac[w[pos]]
                assert e, "no such AC code"
                pos += e >> 8
                r, n = (e & 255) >> 4, e & 15
                if n:
                    k += r
                    assert k < 64, "a run past coefficient 63"
                    x = w[pos] >> (16 - n)
                    pos += n
                    out[zz[k]] = x if x >> (n - 1) else x - (1 << n) + 1
                    k += 1
                elif r == 15:
                    k += 16
                else:
                    break
            assert pos <= s.nbits, "the item ran out of bits"
        if it.end_off >= 0:
            j = it.block0 + it.nblocks
            assert j % bpm == 0 and (j // bpm) % frame.restart == 0 and marker_ahead(s, pos, j // bpm) == it.end_off, "the marker behind the item is not where its row says"
    assert all(w.all() for w in written), "blocks no item decodes"
    return coef


def decode(data, items):
    """the bytes of one file, decoded item by item -> uint8 [H, W, 3]"""
    frame = jpeg.parse(data)
    h, w = frame.height, frame.width
    quant, _ = base.tables_of(frame.tables)
    planes = [base.plane(c, quant[tq]) for c, (tq, _, _) in zip(coefficients(frame, data, items), frame.comp_tables)]
    y = planes[0][:h, :w]
    if frame.sampling == jpeg.GRAY:
        return np.repeat(y[:, :, None], 3, axis=2)
    if frame.sampling == jpeg.S444:
        cb, cr = planes[1][:h, :w], planes[2][:h, :w]
    elif frame.sampling == jpeg.S422:
        cb, cr = (base.upsample_h2v1(p[:h], -(-w // 2), w) for p in planes[1:])
    else:
        cb, cr = (base.upsample_h2v2(p, -(-h // 2), -(-w // 2), h, w) for p in planes[1:])
    return base.ycc_to_rgb(y, cb, cr)
