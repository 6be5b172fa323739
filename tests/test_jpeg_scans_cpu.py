"""vsc_hip.jpeg.parse_scans and the executable contract of vsc_jpeg_decode_scans_u8 (tests/jpeg_scans_contract.py), without a GPU:
on every case of tests/jpeg_scans_cases.py the contract equals Pillow byte for byte, and on the progressive ones also the existing
contract applied to the same image saved non-progressively -- a complete progressive file ends with its sequential twin's
coefficients, so its pixels are the existing contract's.  Scan scripts libjpeg would warn about, unfinished and truncated files
are refused by name, and jpeg.parse refuses every one of them exactly as it did."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_decode_cases as single  # noqa: E402
import jpeg_decode_contract as base  # noqa: E402
import jpeg_scans_cases as cases  # noqa: E402
import jpeg_scans_contract as contract  # noqa: E402
from jpeg_decode_contract import jpeg  # noqa: E402


@pytest.mark.parametrize("name", cases.names())
def test_contract_equals_pillow(name):
    data = cases.file(name)
    frame = jpeg.parse_scans(data)
    assert isinstance(frame, jpeg.ScanFrame), frame
    assert isinstance(jpeg.parse(data), jpeg.Refusal) and jpeg.parse(data).reason in ("progressive", "multiple_scans", "huffman_table_id")
    got, want = cases.contract(name), cases.pillow(name)
    assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))


@pytest.mark.parametrize("name", cases.GRID)
def test_progressive_file_has_its_sequential_twins_pixels(name):
    twin = cases.twin(name)
    assert isinstance(jpeg.parse(twin), jpeg.Frame)
    assert np.array_equal(cases.contract(name), base.decode(twin)), name


def test_the_grid_crosses_sizes_samplings_qualities_and_contents():
    assert len(cases.GRID) == 7 * 4 * 3 * 3
    scripts = {len(jpeg.parse_scans(cases.file(n)).scans) for n in cases.GRID}
    assert scripts == {6, 10}                         # Pillow's scripts: one component, three components
    # 13 x 17 in 4:2:0: chroma is 1 x 2 blocks in its own scans and 2 x 2 in the MCU grid
    f = jpeg.parse_scans(cases.file("13x17_420_q75_noise"))
    _, _, mx, my, comps = contract.geometry(f)
    assert (mx, my) == (2, 1) and comps[1][2:] == (2, 1) and comps[0][2:] == (3, 2)
    # optimised files carry tables of their own per scan
    f = jpeg.parse_scans(cases.file("33x47_420_optimize"))
    assert len({s.tables for s in f.scans}) > 3
    assert jpeg.parse_scans(cases.file("33x47_420_restart_3_blocks")).scans[0].restart == 3


def test_parse_scans_returns_parses_frame_where_parse_accepts():
    for name in ("8x8_444", "37x53_gray", "64x48_restart_2_mcus", "37x53_optimize"):
        for data in single.files(name):
            assert jpeg.parse_scans(data) == jpeg.parse(data) and isinstance(jpeg.parse(data), jpeg.Frame)
    for data, reason in single.refusals().values():
        assert jpeg.parse(data).reason == reason


def test_handmade_scripts():
    f = jpeg.parse_scans(cases.file("33x47_420_one_scan_per_component"))
    assert not f.progressive and [(s.comps, s.ss, s.se) for s in f.scans] == [((0,), 0, 63), ((1,), 0, 63), ((2,), 0, 63)]
    assert jpeg.parse(cases.file("33x47_420_one_scan_per_component")).reason == "multiple_scans"
    f = jpeg.parse_scans(cases.file("33x47_420_table_ids_2_3"))
    assert len(f.scans) == 1 and f.scans[0].huff == ((2, 2), (3, 3), (3, 3))
    assert jpeg.parse(cases.file("33x47_420_table_ids_2_3")).reason == "huffman_table_id"
    f = jpeg.parse_scans(cases.file("33x47_420_dht_redefined"))
    assert [s.huff for s in f.scans] == [((0, 0),)] * 3 and f.scans[0].tables != f.scans[1].tables and f.scans[1].tables == f.scans[2].tables


@pytest.mark.parametrize("name", sorted(cases.refused()))
def test_refusals_by_name(name):
    data, reason, today = cases.refused()[name]
    got = jpeg.parse_scans(data)
    assert isinstance(got, jpeg.Refusal) and got.reason == reason and reason in jpeg.REASONS, got
    assert jpeg.parse(data) == today


def test_more_scripts_are_refused():
    whole = cases._progressive_420()
    head, scans, tail = cases.pieces(whole)
    # a scan sent twice; a DC scan of coefficients 0 .. 5; Al 14; an AC scan of two components
    assert jpeg.parse_scans(head + scans[0] + scans[0] + b"".join(scans[1:]) + tail).reason == "scan_script"

    def patched(i, at, value):
        s = bytearray(scans[i])
        s[s.index(b"\xff\xda") + at] = value
        return head + b"".join(scans[:i]) + bytes(s) + b"".join(scans[i + 1:]) + tail
    assert jpeg.parse_scans(patched(0, 12, 5)).reason == "scan_script"          # Se of the DC scan
    assert jpeg.parse_scans(patched(1, 9, 0x0E)).reason == "scan_script"        # Al 14
    assert jpeg.parse_scans(patched(1, 8, 64)).reason == "scan_script"          # Se 64
    assert jpeg.parse_scans(whole[:-2]).reason == "truncated_scans"              # no EOI
    one = cases.file("33x47_420_one_scan_per_component")
    h, s, t = cases.pieces(one)
    assert jpeg.parse_scans(h + s[0] + s[1] + t).reason == "incomplete_scans"    # no Cr scan
    assert jpeg.parse_scans(h + s[0] + s[1] + s[1] + s[2] + t).reason == "scan_script"
    # a quantisation table behind the first scan
    dqt = whole[whole.index(b"\xff\xdb"):]
    dqt = dqt[:2 + (dqt[2] << 8 | dqt[3])]
    assert jpeg.parse_scans(head + scans[0] + dqt + b"".join(scans[1:]) + tail).reason == "quant_redefined"


def test_contract_statuses_of_the_damaged_files():
    st = {k: v[1] for k, v in cases.damaged().items()}
    assert st == {"flipped_bit_in_ac_refine": contract.RUN, "scan_shortened_by_one_byte": contract.DATA, "eobrun_past_the_last_block": contract.RUN,
                  "wrong_rst": contract.RESTART}


def test_a_single_scan_frame_as_a_scan_list_is_the_existing_contract():
    for name in ("17x9_420", "37x53_gray", "64x48_restart_2_mcus", "37x53_optimize"):
        for data, want in zip(single.files(name), single.contract(name)):
            got, status = contract.decode_frame(jpeg.parse(data), data)
            assert status == 0 and np.array_equal(got, want)
    want = {"scan_cut_at_a_third": 1, "deleted_rst": 4}
    for name, status in want.items():
        data = single.corrupt()[name]
        assert contract.decode_frame(jpeg.parse(data), data)[1] == status


def test_table_sets_and_rows():
    files = [cases.file("13x17_420_q75_noise"), single.files("8x8_444")[0], cases.file("33x47_420_dht_redefined")]
    data, rows, srows, ptr, tables, out_len, outs = cases.call(files, 1, 5)
    assert rows.shape == (3, jpeg.FRAME_ROW) and srows.shape == (14, jpeg.SCAN_ROW) and ptr.tolist() == [0, 10, 11, 14]
    assert tables.shape[1] == jpeg.SCAN_TABLE_SET_BYTES == 2696 and out_len == 1 + sum(h * w * 3 + 5 for _, h, w in outs)
    assert srows[10].tolist()[2:8] == [7, 0, 63, 0, 0, 0] and srows[0].tolist()[2:7] == [7, 0, 0, 0, 1]
    blob = jpeg.widen_tables(jpeg.parse(files[1]).tables)
    assert len(blob) == jpeg.SCAN_TABLE_SET_BYTES and blob[2689] == 0x33
