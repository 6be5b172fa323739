"""``--decode hip`` without a GPU: the numpy contract (tests/jpeg_decode_contract.py) equals Pillow's decode bit for bit on every
well-formed case of tests/jpeg_decode_cases.py, none of which the parser (vsc_hip/jpeg.py) may refuse; the parser's records, its
named refusals, the de-duplication of table sets, and the loaders' ``raw="bytes"`` items."""
import io
import os
import struct
import sys
import zipfile

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "vsc22-submission_amd"))

import jpeg_decode_cases as cases  # noqa: E402
from vsc_hip import jpeg  # noqa: E402


def test_no_well_formed_case_is_refused():
    refused = [(n, i, r) for n in cases.names() for i, r in enumerate(jpeg.parse(f) for f in cases.files(n)) if not isinstance(r, jpeg.Frame)]
    assert len(refused) == 0, refused
    classes = {jpeg.parse(f).sampling for n in cases.names() for f in cases.files(n)}
    assert classes == {jpeg.GRAY, jpeg.S444, jpeg.S422, jpeg.S420}


@pytest.mark.parametrize("name", cases.names())
def test_contract_equals_pillow(name):
    got, want = cases.contract(name), cases.pillow(name)
    assert len(got) == len(want) == len(cases.files(name))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.uint8 and a.shape == b.shape, (name, i, a.shape, b.shape)
        assert np.array_equal(a, b), (name, i, int((a != b).sum()), np.argwhere(a != b)[:4].tolist())


def test_cases_cover_what_they_claim():
    """the encoder wrote what the case names say: restart intervals, custom tables, the box-upsampling sizes, stuffed bytes"""
    f = jpeg.parse(cases.files("64x48_restart_2_mcus")[0])
    assert f.restart == 2 and cases.files("64x48_restart_2_mcus")[0].count(b"\xff\xd0") >= 1
    rows = jpeg.parse(cases.files("64x48_restart_mcu_row")[0])
    assert rows.restart == 3 and rows.sampling == jpeg.S420                       # 48 columns: three MCUs a row
    default = jpeg.parse(cases.files("37x53_420")[0]).tables
    assert all(jpeg.parse(f).tables != default for f in cases.files("37x53_optimize"))
    for name in ("1x1_420", "5x3_422", "4x4_420"):
        f = jpeg.parse(cases.files(name)[0])
        assert -(-f.width // 2) <= 2, name                                        # plain replication instead of the triangle filter
    assert -(-jpeg.parse(cases.files("3x5_420")[0]).width // 2) == 3             # the narrowest chroma the triangle filter takes
    noisy = cases.files("noise_q100")[0]
    f = jpeg.parse(noisy)
    assert noisy[f.seg_start:f.seg_end].count(b"\xff\x00") > 10
    assert len(cases.files("mixed70")) == 70 and len({(p.height, p.width, p.sampling) for p in map(jpeg.parse, cases.files("mixed70"))}) > 20


def test_record_fields():
    data = cases.files("37x53_420")[0]
    f = jpeg.parse(data)
    assert (f.height, f.width, f.sampling, f.restart) == (37, 53, jpeg.S420, 0)
    assert f.comp_tables == ((0, 0, 0), (1, 1, 1), (1, 1, 1)) and f.comp_word == 0 | (1 | 1 << 2 | 1 << 3) << 8 | (1 | 1 << 2 | 1 << 3) << 16
    assert data[f.seg_end:f.seg_end + 2] == b"\xff\xd9" and f.seg_end == len(data) - 2
    sos = data.rindex(b"\xff\xda", 0, f.seg_start)
    assert f.seg_start == sos + 2 + struct.unpack(">H", data[sos + 2:sos + 4])[0]
    assert len(f.tables) == jpeg.TABLE_SET_BYTES and f.tables[1600] == 0b11 and f.tables[1601] == 0b1111
    g = jpeg.parse(cases.files("37x53_gray")[0])
    assert g.sampling == jpeg.GRAY and g.comp_tables == ((0, 0, 0),) and g.tables[1600] == 1 and g.tables[1601] == 0b0101
    assert jpeg.parse(np.frombuffer(data, np.uint8)) == f and jpeg.parse(bytearray(data)) == f
    cut = jpeg.parse(cases.corrupt()["scan_cut_at_a_third"])                     # a header that parses: the scan runs to the end of the file
    assert isinstance(cut, jpeg.Frame) and cut.seg_end == len(cases.corrupt()["scan_cut_at_a_third"])


def test_table_sets_are_shared_by_content():
    data, rows, tables, out_len, outs = cases.call(cases.files("mixed70"))
    assert tables.shape == (3, jpeg.TABLE_SET_BYTES) and sorted(set(rows[:, 6].tolist())) == [0, 1, 2]
    assert len({t.tobytes() for t in tables}) == 3
    sets = jpeg.TableSets()
    a, b = (jpeg.parse(cases.files(n)[0]) for n in ("37x53_420", "17x9_422"))     # two encodes with the default tables at quality 75
    assert sets.add(a.tables) == sets.add(b.tables) == 0 and len(sets) == 1
    assert sets.add(jpeg.parse(cases.files("37x53_optimize")[0]).tables) == 1
    assert out_len == sum(h * w * 3 for _, h, w in outs) and rows.dtype == np.int64 and rows.shape == (70, jpeg.FRAME_ROW)
    offsets = np.cumsum([0] + [len(f) for f in cases.files("mixed70")])
    for r, f, at in zip(rows, cases.files("mixed70"), offsets):
        p = jpeg.parse(f)
        assert r[0] == at + p.seg_start and r[1] == p.seg_end - p.seg_start and tuple(r[2:6]) == (p.height, p.width, p.sampling, p.restart)
    assert bytes(data) == b"".join(cases.files("mixed70"))


def _with_segment(data, marker, payload, before=b"\xff\xdb"):
    at = data.index(before)
    return data[:at] + b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload + data[at:]


def _without_segment(data, marker):
    at = data.index(b"\xff" + bytes([marker]))
    return data[:at] + data[at + 2 + struct.unpack(">H", data[at + 2:at + 4])[0]:]


def test_refusals_name_their_reason():
    for name, (data, reason) in cases.refusals().items():
        r = jpeg.parse(data)
        assert isinstance(r, jpeg.Refusal) and r.reason == reason and r.message, (name, r)
    whole = cases.files("37x53_420")[0]
    sof = whole.index(b"\xff\xc0")

    def patched(at, value):
        b = bytearray(whole)
        b[at] = value
        return bytes(b)

    want = {
        "arithmetic": patched(sof + 1, 0xC9), "lossless": patched(sof + 1, 0xC3), "hierarchical": patched(sof + 1, 0xC5),
        "precision": patched(sof + 4, 12),
        "sampling": patched(sof + 11, 0x12),                                                 # luma 1 x 2: 4:4:0
        "adobe_rgb": _with_segment(whole, 0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00"),
        "missing_tables": _without_segment(whole, 0xC4),
        "quant16": _with_segment(whole, 0xDB, b"\x12" + b"\x00\x01" * 64),
        "huffman_table_id": _with_segment(whole, 0xC4, b"\x02" + b"\x01" + b"\x00" * 15 + b"\x00"),
        "not_jpeg": b"\x89PNG\r\n\x1a\n" + whole,
        "multiple_scans": whole[:-2] + whole[whole.rindex(b"\xff\xda"):],                    # a second SOS behind the first scan
    }
    for reason, data in want.items():
        r = jpeg.parse(data)
        assert isinstance(r, jpeg.Refusal) and r.reason == reason and r.reason in jpeg.REASONS, (reason, r)
    for cut in (1, 3, sof + 5, whole.rindex(b"\xff\xda") + 3):
        r = jpeg.parse(whole[:cut])
        assert isinstance(r, jpeg.Refusal) and r.reason in ("truncated_header", "not_jpeg"), (cut, r)
    two = bytearray(whole)                                                                   # a scan of one of the three components
    sos = whole.rindex(b"\xff\xda")
    two[sos + 4] = 1
    assert jpeg.parse(bytes(two)).reason in ("multiple_scans", "bad_header")
    assert isinstance(jpeg.parse(_with_segment(whole, 0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01")), jpeg.Frame)       # transform 1: YCbCr


def _zip(path, frames):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with zipfile.ZipFile(path, "w") as z:
        for i, data in enumerate(frames):
            z.writestr(f"{i:05d}.jpg", data)


def test_loader_items_carry_bytes_or_fall_back_whole(tmp_path):
    """ZipFrames(raw="bytes"): (bytes, offsets, records, video_id) for a video the device can take; the host-decoded frames, as
    ``raw=True`` gives them, for a video with a refused frame or with frames of two sizes"""
    import torch
    from src.dataset import BytesVideo, ZipFrames, vit_transform_u8
    rng = np.random.default_rng(5)
    enc = lambda h, w, **kw: cases.encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "420", **kw)     # noqa: E731
    videos = {"R000001": [enc(48, 64) for _ in range(4)], "R000002": [enc(48, 64), enc(48, 64, progressive=True), enc(48, 64)],
              "R000003": [enc(48, 64), enc(40, 40)]}
    for vid, frames in videos.items():
        _zip(os.path.join(str(tmp_path), vid[-2:], vid + ".zip"), frames)
    t = vit_transform_u8(32, 32)
    ds = ZipFrames(list(videos), str(tmp_path), t, raw="bytes")
    host = ZipFrames(list(videos), str(tmp_path), t, raw=True)
    item, vid = ds[0]
    assert vid == "R000001" and isinstance(item, BytesVideo) and item.shape == (4, 48, 64)
    assert item.data.dtype == torch.uint8 and bytes(item.data.numpy()) == b"".join(videos[vid])
    assert item.offsets.tolist() == np.cumsum([0] + [len(f) for f in videos[vid]]).tolist()
    assert all(isinstance(r, jpeg.Frame) and (r.height, r.width) == (48, 64) for r in item.records)
    import pickle
    back = pickle.loads(pickle.dumps(item))                         # a loader worker sends the item to the main process pickled
    assert torch.equal(back.data, item.data) and back.offsets.tolist() == item.offsets.tolist() and back.records == item.records
    for i in (1, 2):
        got, want = ds[i], host[i]
        assert isinstance(got[0], torch.Tensor) and got[1] == want[1] and torch.equal(got[0], want[0])
