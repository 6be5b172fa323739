"""JPEG decoding in parallel inside a frame on the device (csrc/jpeg_split.hip, ops.jpeg_decode(split=), ``--decode_split`` of
both extraction entry points): vsc_jpeg_decode_split_u8 through ctypes on every well-formed case of tests/jpeg_split_cases.py --
restart-marker frames at three item sizes, sub-stream frames at 64 bytes with as many rounds as sub-streams, the frame that falls
back with one round, the 360 x 640 frame at the defaults -- between 0xFF guard bands, against the executable contract
(tests/jpeg_split_contract.py: bytes and the four statistics) and against Pillow, bit for bit; one mixed call at odd addresses,
chunked, three times on one handle; the refusals; and both entry points with ``--decode hip --decode_split all`` against
``--decode hip``, byte for byte.  Damaged scans are not run here: tests/test_jpeg_split_emulated.py runs them on the same source."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_decode_cases as cases  # noqa: E402
import jpeg_split_cases as sc  # noqa: E402
import jpeg_split_contract as contract  # noqa: E402
from vsc_hip import jpeg  # noqa: E402

pytestmark = pytest.mark.gpu

P, I64 = ctypes.c_void_p, ctypes.c_int64


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def nsub(data, sub_bytes=sc.SUB_BYTES):
    f = jpeg.parse(data)
    return -(-(f.seg_end - f.seg_start) // sub_bytes)


def run_entry(file_list, dev, split=(3, 0, 0, 0), guard=509, fill=0x5A, cap=0, gap=5, restarts=None, null_handle=False, repeat=1, mutate=None):
    """``repeat`` vsc_jpeg_decode_split_u8 calls on one handle and the null stream: [guard | bytes | guard | output | guard | status |
    guard] in one arena -> (rc, status, [frame], chunks, stats, everything else intact and every repeat the same bits)"""
    from vsc_hip import _lib
    lib = _lib.load()
    data, rows, tables, out_len, outs, ptr, off = sc.call(file_list, 0, gap, restarts)
    if mutate is not None:
        ptr, off = mutate(ptr, off)
    n = len(rows)
    st_at = (3 * guard + len(data) + out_len + 3) & ~3
    d_at, o_at = guard, 2 * guard + len(data)
    hd = P()
    _lib.check(lib.vsc_jpeg_decode_create(None, ctypes.byref(hd)))
    chunks, stats, intact, first = I64(-1), np.full(4, -1, np.int64), True, None
    try:
        if cap:
            _lib.check(lib.vsc_jpeg_decode_scratch(hd, cap, None, None))
        _lib.check(lib.vsc_jpeg_decode_split(hd, *split))
        for _ in range(repeat):
            arena = torch.full((st_at + 4 * n + guard,), 0xFF, dtype=torch.uint8, device=dev)
            arena[d_at:d_at + len(data)] = torch.from_numpy(data.copy()).to(dev)
            arena[o_at:o_at + out_len] = fill
            arena[st_at:st_at + 4 * n] = 0x77
            base = arena.data_ptr()
            rc = lib.vsc_jpeg_decode_split_u8(None if null_handle else hd, P(base + d_at), len(data), rows.ctypes.data, n, tables.ctypes.data, len(tables),
                                              ptr.ctypes.data if ptr is not None else None, off.ctypes.data if off is not None and len(off) else None,
                                              P(base + o_at), out_len, P(base + st_at))
            if rc == 0:
                _lib.check(lib.vsc_jpeg_decode_stats(hd, stats.ctypes.data))
            torch.cuda.synchronize()
            host = arena.cpu().numpy()
            out = host[o_at:o_at + out_len]
            keep = np.ones(out_len, bool)
            for at, h, w in outs:
                keep[at:at + h * w * 3] = False
            intact = intact and bool((host[:d_at] == 0xFF).all() and np.array_equal(host[d_at:d_at + len(data)], data) and (host[d_at + len(data):o_at] == 0xFF).all()
                                     and (host[o_at + out_len:st_at] == 0xFF).all() and (host[st_at + 4 * n:] == 0xFF).all() and (out[keep] == fill).all())
            if first is None:
                first = host
            intact = intact and np.array_equal(first, host)
        _lib.check(lib.vsc_jpeg_decode_scratch(hd, 0, ctypes.byref(chunks), None))
    finally:
        lib.vsc_jpeg_decode_destroy(hd)
    status = host[st_at:st_at + 4 * n].copy().view(np.int32)
    return rc, status, [out[at:at + h * w * 3].reshape(h, w, 3) for at, h, w in outs], chunks.value, tuple(int(v) for v in stats), intact


def check_frames(frames, file_list, references):
    for i, (got, data, ref) in enumerate(zip(frames, file_list, references)):
        bad = int((got != ref).sum())
        if bad or i == 0:
            print(f"frame {i} {got.shape}: {bad} bytes differ from the contract")
        assert np.array_equal(got, ref), (i, bad, np.argwhere(got != ref)[:4].tolist())
        assert np.array_equal(got, pillow(data)), (i, "differs from Pillow")


@pytest.mark.parametrize("item_bytes", sc.ITEM_BYTES)
@pytest.mark.parametrize("name", sorted(sc.marker()))
def test_marker_items_equal_contract_and_pillow(dev, name, item_bytes):
    from vsc_hip import _lib
    data = sc.marker()[name][0]
    want = contract.split(data, item_bytes=item_bytes)
    rc, status, frames, chunks, stats, intact = run_entry([data], dev, split=(3, 0, 0, item_bytes))
    assert rc == 0, _lib.load().vsc_last_error()
    assert intact, "a guard band, a gap or the input was written"
    assert status.tolist() == [0] and chunks == 1
    check_frames(frames, [data], [sc.reference(name)])
    print(f"{name} item_bytes {item_bytes}: statistics {stats}, contract {contract.stats([want])}")
    assert want.kind == "markers" and stats == contract.stats([want])


@pytest.mark.parametrize("name", sorted(sc.substream()))
def test_substreams_equal_contract_and_pillow(dev, name):
    """64-byte sub-streams and as many rounds as there are sub-streams: every frame is cut, none falls back"""
    from vsc_hip import _lib
    data = sc.substream()[name]
    rounds = nsub(data)
    want = contract.split(data, sc.SUB_BYTES, rounds)
    rc, status, frames, _, stats, intact = run_entry([data], dev, split=(3, sc.SUB_BYTES, rounds, 0))
    assert rc == 0, _lib.load().vsc_last_error()
    assert intact and status.tolist() == [0]
    check_frames(frames, [data], [sc.reference(name)])
    print(f"{name}: {rounds} sub-streams, statistics {stats}, contract {contract.stats([want])}")
    assert want.kind == "substreams" and stats == (0, 1, 0, rounds) == contract.stats([want])


def test_one_round_falls_back_where_the_contract_does(dev):
    """noise_q100[0] at 32 bytes a sub-stream: few states are right after the speculative round; one item, the same bytes"""
    data = cases.files("noise_q100")[0]
    want = contract.split(data, 32, 1)
    rc, status, frames, _, stats, intact = run_entry([data], dev, split=(3, 32, 1, 0))
    assert rc == 0 and intact and status.tolist() == [0]
    check_frames(frames, [data], [cases.contract("noise_q100")[0]])
    print(f"noise_q100[0]: {want.right_after_round0} of {len(want.exits[0])} states right after round 0; statistics {stats}")
    assert want.kind == "fallback" and stats == (0, 0, 1, len(want.exits[0])) == contract.stats([want])


def test_360x640_at_the_defaults(dev):
    data = cases.files("360x640_420")[0]
    want = contract.split(data)
    rc, status, frames, _, stats, intact = run_entry([data], dev, split=(3, 0, 0, 0))
    assert rc == 0 and intact and status.tolist() == [0]
    check_frames(frames, [data], [cases.contract("360x640_420")[0]])
    print(f"360x640_420 at {jpeg.SPLIT_SUB_BYTES} bytes, {jpeg.SPLIT_ROUNDS} rounds: statistics {stats}, contract {contract.stats([want])}")
    assert stats == contract.stats([want])
    assert want.kind == "substreams" and stats[1] == 1 and stats[2] == 0, "the contract itself says: cut, no fallback"


def test_mixed_call_chunked_three_runs(dev):
    """marker frames, sub-stream frames, a one-component frame and 1 x 1 frames in one call at odd addresses with gaps, in chunks
    under a cap of 9000 bytes of planes, three times on one handle"""
    files = sc.mixed()
    want = [contract.split(f, sc.SUB_BYTES, 8, 300) for f in files]
    rc, status, frames, chunks, stats, intact = run_entry(files, dev, split=(3, sc.SUB_BYTES, 8, 300), guard=509, gap=5, cap=9000, repeat=3)
    assert rc == 0 and intact and (status == 0).all() and chunks > 2, (status.tolist(), chunks)
    check_frames(frames, files, sc.mixed_reference())
    assert stats == contract.stats(want) and stats[0] == 4 and stats[1] == 4 and stats[2] == 1, (stats, contract.stats(want))
    for mode in (0, 1, 2):                                        # only what the mode names is cut
        want = [contract.split(f, sc.SUB_BYTES, 8, 300, mode) for f in files]
        rc, status, frames, _, stats, intact = run_entry(files, dev, split=(mode, sc.SUB_BYTES, 8, 300), guard=512, gap=0)
        assert rc == 0 and intact and (status == 0).all() and stats == contract.stats(want), (mode, stats)
        assert all(np.array_equal(a, b) for a, b in zip(frames, sc.mixed_reference()))


def test_refusals_launch_nothing(dev):
    from vsc_hip import _lib
    lib = _lib.load()
    files = [sc.marker()["40x56_420_interval_5"][0], sc.substream()["37x53_gray"]]

    def refused(**kw):
        rc, status, frames, _, _, intact = run_entry(files, dev, **kw)
        assert rc != 0
        assert intact and all((f == 0x5A).all() for f in frames) and (status == 0x77777777).all(), "a refused call wrote"

    refused(null_handle=True)
    seg = jpeg.parse(files[0])
    seg_len = seg.seg_end - seg.seg_start
    refused(restarts={0: [10, 5]})                                 # not ascending
    refused(restarts={0: [10, 11]})                                # closer than a marker is long
    refused(restarts={0: [-1, 40]})
    refused(restarts={0: [10, seg_len - 1]})                       # the marker would end outside the segment
    refused(restarts={1: [1 << 20]})                               # checked for every frame, with a restart interval or without
    refused(mutate=lambda ptr, off: (ptr + 1, off))                # rows that do not start at 0
    refused(mutate=lambda ptr, off: (ptr[::-1].copy(), off))       # descending rows
    hd = P()
    _lib.check(lib.vsc_jpeg_decode_create(None, ctypes.byref(hd)))
    try:
        for bad in ((4, 0, 0, 0), (-1, 0, 0, 0), (3, 16, 0, 0), (3, 66, 0, 0), (3, 0, 129, 0), (3, 0, -1, 0), (3, 0, 0, -1)):
            assert lib.vsc_jpeg_decode_split(hd, *bad) != 0, bad
        assert lib.vsc_jpeg_decode_split(None, 3, 0, 0, 0) != 0 and lib.vsc_jpeg_decode_stats(hd, None) != 0
    finally:
        lib.vsc_jpeg_decode_destroy(hd)
    # a row with another number of offsets than the frame's interval asks for is no refusal: the frame is one item
    rc, status, frames, _, stats, intact = run_entry(files, dev, split=(3, sc.SUB_BYTES, 13, 1), restarts={0: [10]})
    assert rc == 0 and intact and (status == 0).all() and stats == (0, 1, 1, 14)
    check_frames(frames, files, [sc.reference("40x56_420_interval_5"), sc.reference("37x53_gray")])


def test_ops_jpeg_decode_split_on_a_side_stream(dev):
    """ops.jpeg_decode(split=) three times on the process's handle: the bits of ops.jpeg_decode without it"""
    from vsc_hip import ops
    files = list(sc.mixed())
    data, rows, tables, out_len, outs, ptr, off = sc.call(files)
    dd = torch.from_numpy(data.copy()).to(dev)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        plain, status = ops.jpeg_decode(dd, rows, tables, out_len)
        assert int(status.abs().sum().item()) == 0
        for split in ("markers", "substreams", "all", {"mode": "all", "sub_bytes": 64, "rounds": 8, "item_bytes": 300}, "none"):
            out, status = ops.jpeg_decode(dd, rows, tables, out_len, restarts=(ptr, off), split=split)
            assert int(status.abs().sum().item()) == 0 and torch.equal(out, plain), split
            if split != "none":
                st = ops.jpeg_decode_stats()
                assert st[0] == (0 if split == "substreams" else 4) and st[1] + st[2] == (0 if split == "markers" else 5), (split, st)
    side.synchronize()
    with pytest.raises(ValueError, match="split must be one of"):
        ops.jpeg_decode(dd, rows, tables, out_len, split="rows")


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
def _setup(tmp_path, prefix):
    """the videos of test_gpu_jpeg_decode plus one whose frames carry a restart marker behind every MCU row"""
    from test_gpu_jpeg_decode import _jpg_zips, _videos
    from test_gpu_uap_e2e import GOLD, _checkpoints, _pca_pickle
    g = np.load(GOLD)
    root = str(tmp_path)
    videos = _videos(prefix, 600001)
    rng = np.random.default_rng(77)
    videos[f"{prefix}{600004:06d}"] = [cases.encode(cases.picture(int(rng.integers(1 << 30)), 48, 64), "420", restart_marker_rows=1) for _ in range(4)]
    zips = os.path.join(root, "zips")
    _jpg_zips(zips, videos)
    ids = os.path.join(root, "ids.txt")
    with open(ids, "w") as f:
        f.write("\n".join(videos) + "\n")
    pca_path = os.path.join(root, "pca_model.pkl")
    _pca_pickle(g, pca_path)
    return root, zips, ids, _checkpoints(g, root), pca_path, videos


def test_extract_ref_feats_decode_split_writes_the_same_file(tmp_path):
    import extract_ref_feats as E
    from test_gpu_frame_inputs import _npz, assert_same_npz
    root, zips, ids, models, _, videos = _setup(tmp_path, "R")
    _, arch, fmt, ckpt = models[1]
    common = ["--zip_prefix", zips, "--input_file", ids, "--checkpoint_path", ckpt, "--arch", arch, "--weights_format", fmt, "--batch_size", "2", "--workers", "0",
              "--resize", "hip"]
    out = {}
    for name, extra in (("plain", ["--decode", "hip"]), ("split", ["--decode", "hip", "--decode_split", "all"])):
        out[name] = os.path.join(root, f"{arch}_{name}")
        E.main(E.build_parser().parse_args(["--save_file", out[name]] + common + extra))
    assert_same_npz(out["split"] + ".npz", out["plain"] + ".npz")
    assert len(_npz(out["split"] + ".npz")["features"]) == sum(len(v) for v in videos.values())
    with pytest.raises(ValueError, match="--decode hip"):
        E.main(E.build_parser().parse_args(["--save_file", out["split"]] + common + ["--decode_split", "all"]))


def test_extract_query_feats_decode_split_writes_the_same_files(tmp_path):
    import extract_query_feats as E
    from test_gpu_frame_inputs import assert_same_npz
    root, zips, ids, models, pca_path, _ = _setup(tmp_path, "Q")
    spec = [f"{arch}:{fmt}:{ckpt}" for _, arch, fmt, ckpt in models]
    keys = [os.path.split(ckpt)[-1].split(".")[0] for _, _, _, ckpt in models]

    def run(name, *extra):
        out = os.path.join(root, name)
        E.main(E.build_parser().parse_args(["--split", "test", "--models"] + spec + ["--pca_model", pca_path, "--zip_prefix", zips, "--input_file", ids,
                                                                                      "--output_dir", out, "--workers", "0", "--resize", "hip", *extra]))
        return out

    plain, split = run("plain", "--decode", "hip"), run("split", "--decode", "hip", "--decode_split", "all")
    for key in keys:
        assert_same_npz(os.path.join(split, key, "test_query.npz"), os.path.join(plain, key, "test_query.npz"))
    assert_same_npz(os.path.join(split, "test_query_sn.npz"), os.path.join(plain, "test_query_sn.npz"))
    with pytest.raises(ValueError, match="--decode hip"):
        run("no", "--decode_split", "markers")


def test_decoder_cuts_the_loaders_videos(dev, tmp_path):
    """ZipFrames(raw="bytes") -> HipDecode(split="all"): the BytesVideo items carry their marker offsets, the call cuts the frames
    (statistics), and the device frames equal the workers' Pillow frames"""
    from src.dataset import BytesVideo, ZipFrames, vit_transform_u8
    from src.image_preprocess import HipDecode
    from test_gpu_jpeg_decode import _jpg_zips, _videos
    from vsc_hip import ops
    videos = _videos("R", 700001)
    _jpg_zips(str(tmp_path), videos)
    t = vit_transform_u8(32, 32)
    packed, host = ZipFrames(list(videos), str(tmp_path), t, raw="bytes"), ZipFrames(list(videos), str(tmp_path), t, raw=True)
    items = [packed[i][0] for i in range(2)]
    assert all(isinstance(v, BytesVideo) for v in items)
    assert int(items[0].restarts[0][-1]) == 0 and int(items[1].restarts[0][-1]) == 4 * 5      # 48 rows of 4:4:4: six MCU rows, five markers a frame
    decoder = HipDecode(dev, split="all")
    frames = decoder(items)
    torch.cuda.current_stream().synchronize()
    for i, f in enumerate(frames):
        assert f.is_cuda and torch.equal(f.cpu(), host[i][0]), i
    with torch.cuda.stream(decoder.stream):
        st = ops.jpeg_decode_stats()
    assert st[0] == 4 and st[1] == 6 and st[2] == 0, st
    with pytest.raises(ValueError, match="decode_split must be one of"):
        HipDecode(dev, split="rows")
