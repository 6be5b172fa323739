"""The contract of vsc_jpeg_decode_split_u8 on the CPU (tests/jpeg_split_contract.py, vsc_hip/jpeg.py's marker scan): however a
frame of tests/jpeg_split_cases.py is cut into items -- at its restart markers with three item sizes, into 64-byte sub-streams --
decoding the items gives Pillow's bytes; the marker scan finds what the encoder wrote and the count rule decides which frames
are cut; the sub-stream rounds converge as the fixed-point argument says; and the options are checked before anything runs."""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_decode_cases as cases  # noqa: E402
import jpeg_split_cases as sc  # noqa: E402
import jpeg_split_contract as contract  # noqa: E402
from vsc_hip import jpeg  # noqa: E402


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", sorted(sc.marker()))
def test_marker_scan_and_items_decode_to_pillow(name):
    data, markers = sc.marker()[name]
    f = jpeg.parse(data)
    off = jpeg.restart_offsets(np.frombuffer(data, np.uint8), f)
    assert len(off) == markers == jpeg.expected_restarts(f)
    seg = data[f.seg_start:f.seg_end]
    assert all(seg[o] == 0xFF and seg[o + 1] == 0xD0 + k % 8 for k, o in enumerate(off.tolist()))
    want = pillow(data)
    assert np.array_equal(sc.reference(name), want)
    counts = []
    for item_bytes in sc.ITEM_BYTES:
        s = contract.split(data, item_bytes=item_bytes)
        assert s.kind == "markers" and np.array_equal(contract.decode(data, s.items), want), item_bytes
        assert s.items[-1].end_off == -1 and all(it.end_off in off.tolist() for it in s.items[:-1])
        assert sum(it.nblocks for it in s.items) == contract.geometry(f)[0] * jpeg.mcus(f)
        counts.append(len(s.items))
    assert counts[0] == markers + 1 and counts[2] == 1 and counts[0] >= counts[1] >= 1
    if markers > 5:
        assert counts[0] > counts[1] > 1, "300 bytes an item: several intervals per item, more than one item"
        assert any(it.block0 // (contract.geometry(f)[0] * f.restart) % 8 for it in contract.split(data, item_bytes=300).items[1:]), "an expected RSTn that starts non-zero"


def test_a_stuffed_zero_stands_directly_before_a_marker():
    data, _ = sc.marker()["noise_q100_every_mcu"]
    f = jpeg.parse(data)
    seg = data[f.seg_start:f.seg_end]
    off = jpeg.restart_offsets(np.frombuffer(data, np.uint8), f).tolist()
    assert any(o >= 2 and seg[o - 2:o] == b"\xff\x00" for o in off)


def test_count_rule_and_marker_rows():
    data, _ = sc.marker()["40x56_420_interval_5"]
    f = jpeg.parse(data)
    off = jpeg.restart_offsets(np.frombuffer(data, np.uint8), f).tolist()
    assert contract.split(data, restarts=off[:-1]).kind == "fallback" and contract.split(data, restarts=off + [off[-1] + 2]).kind == "fallback"
    cut = data[:f.seg_start + off[0]] + data[f.seg_start + off[0] + 2:]                 # a deleted RSTn
    g = jpeg.parse(cut)
    assert len(jpeg.restart_offsets(np.frombuffer(cut, np.uint8), g)) == len(off) - 1 and contract.split(cut).kind == "fallback"
    assert contract.split(data, mode=2).kind == "none" and contract.split(sc.substream()["37x53_gray"], mode=1).kind == "none"
    files = [data, sc.substream()["37x53_gray"], b"not a jpeg"]
    records = [jpeg.parse(x) for x in files]
    ptr, rows = jpeg.restart_rows(files, records)
    assert ptr.tolist() == [0, len(off), len(off), len(off)] and rows.tolist() == off and rows.dtype == np.int32 and ptr.dtype == np.int64
    ptr2, rows2 = jpeg.concat_restart_rows([(ptr, rows), (ptr[:2], rows), (np.zeros(1, np.int64), np.zeros(0, np.int32))])
    assert ptr2.tolist() == [0, len(off), len(off), len(off), 2 * len(off)] and rows2.tolist() == off + off
    assert jpeg.expected_restarts(records[1]) == -1


@pytest.mark.parametrize("name", sorted(sc.substream()))
def test_substreams_converge_and_items_decode_to_pillow(name):
    data = sc.substream()[name]
    f = jpeg.parse(data)
    n = -(-(f.seg_end - f.seg_start) // sc.SUB_BYTES)
    s = contract.split(data, sc.SUB_BYTES, n)
    assert s.kind == "substreams" and s.converged and len(s.items) == n and len(s.exits) == n + 1
    want = pillow(data)
    assert np.array_equal(sc.reference(name), want) and np.array_equal(contract.decode(data, s.items), want)
    truth = s.exits[-1]
    for r, exits in enumerate(s.exits):
        assert exits[:r + 1] == truth[:r + 1], "after round r, sub-streams 0 .. r are true whatever the data"
    need = max([r for r in range(1, n + 1) if s.exits[r] != s.exits[r - 1]] + [0]) + 1
    print(f"{name}: {n} sub-streams, {s.right_after_round0} right after the speculative round, {need} round(s) until a round changes nothing")
    assert contract.split(data, sc.SUB_BYTES, min(need, 128)).kind == "substreams"
    if need > 1:
        assert contract.split(data, sc.SUB_BYTES, need - 1).kind == "fallback"
    # a boundary directly behind an FF (the stuffed zero is the sub-stream's first byte), where the cases have one
    seg = data[f.seg_start:f.seg_end]
    behind = sum(1 for k in range(1, n) if seg[k * sc.SUB_BYTES - 1] == 0xFF)
    if name in ("noise_q75", "checker_q100[0]"):
        assert behind >= 1, "the case no longer has a boundary behind an FF"


def test_sub_stream_counts():
    got = {name: -(-(jpeg.parse(d).seg_end - jpeg.parse(d).seg_start) // sc.SUB_BYTES) for name, d in sc.substream().items()}
    assert {k: got[k] for k in ("37x53_420", "37x53_422", "37x53_444", "37x53_gray", "noise_q75", "checker_q100[0]", "checker_q100[1]", "shorter_than_a_substream")} == \
        {"37x53_420": 17, "37x53_422": 20, "37x53_444": 27, "37x53_gray": 13, "noise_q75": 17, "checker_q100[0]": 59, "checker_q100[1]": 4, "shorter_than_a_substream": 1}


def test_one_round_is_not_enough_for_noise_at_32_bytes():
    data = cases.files("noise_q100")[0]
    s = contract.split(data, 32, 1)
    assert s.kind == "fallback" and not s.converged and s.right_after_round0 < 10 and len(s.items) == len(s.exits[0]) > 100
    assert np.array_equal(contract.decode(data, s.items), cases.pillow("noise_q100")[0])
    assert contract.stats([s]) == (0, 0, 1, len(s.exits[0]))


def test_mixed_call_statistics():
    splits = [contract.split(f, sc.SUB_BYTES, 8, 300) for f in sc.mixed()]
    assert contract.stats(splits)[:3] == (4, 4, 1)
    for f, s, ref in zip(sc.mixed(), splits, sc.mixed_reference()):
        assert np.array_equal(contract.decode(f, s.items), ref)


def test_options_are_checked():
    from src.dataset import DECODE_SPLITS, BytesVideo, bytes_video, check_decode_split
    from vsc_hip import ops
    assert DECODE_SPLITS == jpeg.SPLITS == ("none", "markers", "substreams", "all")
    assert check_decode_split("none", "host") == "none" and check_decode_split("all", "hip") == "all"
    with pytest.raises(ValueError, match="--decode hip"):
        check_decode_split("markers", "host")
    with pytest.raises(ValueError, match="decode_split must be one of"):
        check_decode_split("rows", "hip")
    assert ops.jpeg_decode_split_mode("all") == (3, jpeg.SPLIT_SUB_BYTES, jpeg.SPLIT_ROUNDS, jpeg.SPLIT_ITEM_BYTES)
    assert ops.jpeg_decode_split_mode({"mode": "markers", "item_bytes": 7}) == (1, jpeg.SPLIT_SUB_BYTES, jpeg.SPLIT_ROUNDS, 7)
    import extract_query_feats
    import extract_ref_feats
    for E in (extract_ref_feats, extract_query_feats):
        opt = [a for a in E.build_parser()._actions if a.dest == "decode_split"][0]
        assert opt.default == "none" and tuple(opt.choices) == DECODE_SPLITS and "--decode hip" in opt.help
    video = bytes_video([sc.marker()["40x56_420_interval_5"][0]] * 2)
    assert isinstance(video, BytesVideo) and video.restarts[0].tolist() == [0, 2, 4] and len(video.restarts[1]) == 4
