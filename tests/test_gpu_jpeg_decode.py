"""JPEG frame decoding on the device (csrc/jpeg_decode.hip, ops.jpeg_decode, ``--decode hip`` of both extraction entry points):
the entry through ctypes on every well-formed case of tests/jpeg_decode_cases.py -- the 70-frame call of mixed sizes, sampling
classes and table sets and a 360 x 640 frame included -- between 0xFF guard bands, inputs and outputs at dword-aligned and at odd
addresses, against the executable contract (tests/jpeg_decode_contract.py) and against Pillow, bit for bit; a chunked call; three
runs of one call; the refusals; and both entry points with ``--decode hip --resize hip`` against ``--resize hip``, byte for byte.
Damaged scans are not run here: their bounds logic is the same source that tests/test_jpeg_decode_emulated.py runs under the
sanitizers."""
import ctypes
import os
import sys
import zipfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_decode_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

P, I64 = ctypes.c_void_p, ctypes.c_int64


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def run_entry(file_list, dev, guard=512, fill=0x5A, cap=0, gap=0, mutate=None, handle="own"):
    """one vsc_jpeg_decode_u8 call on the null stream: [guard | bytes | guard | output | guard | status | guard] in one arena, the
    frames packed from the output's start with ``gap`` bytes between them -> (rc, status, [frame], chunks, everything else intact)"""
    from vsc_hip import _lib
    lib = _lib.load()
    data, rows, tables, out_len, outs = cases.call(file_list, 0, gap)
    if mutate is not None:
        mutate(rows, tables)
    n = len(rows)
    st_at = (3 * guard + len(data) + out_len + 3) & ~3        # the status array is int32: aligned whatever the rest is
    arena = torch.full((st_at + 4 * n + guard,), 0xFF, dtype=torch.uint8, device=dev)
    d_at, o_at = guard, 2 * guard + len(data)
    arena[d_at:d_at + len(data)] = torch.from_numpy(data.copy()).to(dev)
    arena[o_at:o_at + out_len] = fill
    arena[st_at:st_at + 4 * n] = 0x77
    base = arena.data_ptr()
    hd = P()
    _lib.check(lib.vsc_jpeg_decode_create(None, ctypes.byref(hd)))
    chunks = I64(-1)
    try:
        if cap:
            _lib.check(lib.vsc_jpeg_decode_scratch(hd, cap, None, None))
        rc = lib.vsc_jpeg_decode_u8(hd if handle == "own" else handle, P(base + d_at), len(data), rows.ctypes.data, n, tables.ctypes.data, len(tables),
                                    P(base + o_at), out_len, P(base + st_at))
        _lib.check(lib.vsc_jpeg_decode_scratch(hd, 0, ctypes.byref(chunks), None))
        torch.cuda.synchronize()
    finally:
        lib.vsc_jpeg_decode_destroy(hd)
    host = arena.cpu().numpy()
    out = host[o_at:o_at + out_len]
    keep = np.ones(out_len, bool)
    for at, h, w in outs:
        keep[at:at + h * w * 3] = False
    intact = bool((host[:d_at] == 0xFF).all() and np.array_equal(host[d_at:d_at + len(data)], data) and (host[d_at + len(data):o_at] == 0xFF).all()
                  and (host[o_at + out_len:st_at] == 0xFF).all() and (host[st_at + 4 * n:] == 0xFF).all() and (out[keep] == fill).all())
    status = host[st_at:st_at + 4 * n].copy().view(np.int32)
    return rc, status, [out[at:at + h * w * 3].reshape(h, w, 3) for at, h, w in outs], chunks.value, intact


@pytest.mark.parametrize("guard", [512, 509])
@pytest.mark.parametrize("name", cases.names())
def test_entry_equals_contract_and_pillow(dev, name, guard):
    from vsc_hip import _lib
    rc, status, frames, chunks, intact = run_entry(cases.files(name), dev, guard=guard, gap=0 if guard % 4 == 0 else 5)
    assert rc == 0, _lib.load().vsc_last_error()
    assert intact, "a guard band, a gap or the input was written"
    assert (status == 0).all(), status.tolist()
    want, pil = cases.contract(name), cases.pillow(name)
    assert len(frames) == len(want) == len(pil) and chunks == (1 if want else 0)
    for i, (got, ref, p) in enumerate(zip(frames, want, pil)):
        bad = int((got != ref).sum())
        if bad or i == 0:
            print(f"{name} frame {i} {got.shape}: {bad} bytes differ from the contract")
        assert np.array_equal(got, ref), (name, i, bad, np.argwhere(got != ref)[:4].tolist())
        assert np.array_equal(got, p), (name, i, "differs from Pillow")


def test_chunked_call(dev):
    """five small frames under a scratch cap of 3500 bytes: (768 + 1728) + 2048 + (2304 + 1152) bytes of planes -> three chunks"""
    rc, status, frames, chunks, intact = run_entry(cases.files("five_small"), dev, guard=509, cap=3500, gap=3)
    assert rc == 0 and intact and (status == 0).all() and chunks == 3
    assert all(np.array_equal(a, b) for a, b in zip(frames, cases.pillow("five_small")))


def test_three_runs_give_the_same_bits(dev):
    """the 70-frame call through ops.jpeg_decode on a side stream, three times on one handle"""
    from vsc_hip import ops
    data, rows, tables, out_len, outs = cases.call(cases.files("mixed70"))
    dd = torch.from_numpy(data.copy()).to(dev)
    side = torch.cuda.Stream()
    runs = []
    for _ in range(3):
        with torch.cuda.stream(side):
            out, status = ops.jpeg_decode(dd, rows, tables, out_len)
        side.synchronize()
        assert int(status.abs().sum()) == 0
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    for (at, h, w), p in zip(outs, cases.pillow("mixed70")):
        assert np.array_equal(runs[0][at:at + h * w * 3].reshape(h, w, 3), p)


def test_refusals_launch_nothing(dev):
    from vsc_hip import jpeg
    for name, (data, reason) in cases.refusals().items():        # the parser's: such a file never reaches the entry
        r = jpeg.parse(data)
        assert isinstance(r, jpeg.Refusal) and r.reason == reason, name
    files = cases.files("five_small")

    def refused(mutate=None, **kw):
        rc, status, frames, _, intact = run_entry(files, dev, fill=0x5A, mutate=mutate, **kw)
        assert rc != 0
        assert intact and all((f == 0x5A).all() for f in frames) and (status == 0x77777777).all(), "a refused call wrote"

    def setter(row, col, value):
        def mutate(rows, tables):
            rows[row, col] = value
        return mutate

    refused(handle=None)
    for row, col, value in ((0, 0, -1), (4, 1, 1 << 40), (2, 2, 0), (2, 3, 16385), (1, 4, 4), (3, 5, -1), (0, 6, 9), (4, 7, -1), (4, 7, 1 << 40),
                            (0, 8, 3), (0, 8, 1 << 30)):
        refused(setter(row, col, value))                        # a bad frame row, after good ones too: nothing launched

    def no_prefix_code(rows, tables):
        tables[0, 512] = 3                                      # three codes of length 1
    refused(no_prefix_code)
    rc, status, frames, chunks, intact = run_entry(files, dev)   # and the entry still works
    assert rc == 0 and intact and (status == 0).all() and all(np.array_equal(a, b) for a, b in zip(frames, cases.contract("five_small")))


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
def _jpg_zips(root, videos):
    for vid, frames in videos.items():
        d = os.path.join(root, vid[-2:])
        os.makedirs(d, exist_ok=True)
        with zipfile.ZipFile(os.path.join(d, f"{vid}.zip"), "w") as z:
            for i, data in enumerate(frames):
                z.writestr(f"{i:04d}.jpg", data)


def _videos(prefix, start):
    """videos of 48 x 64 frames in 4:2:0, 4:4:4 with a restart interval and gray; the last one has a progressive frame and stays
    with the host decoder as a whole"""
    rng = np.random.default_rng(start)
    pic = lambda gray=False: cases.picture(int(rng.integers(1 << 30)), 48, 64, gray=gray)     # noqa: E731
    return {f"{prefix}{start:06d}": [cases.encode(pic(), "420") for _ in range(5)],
            f"{prefix}{start + 1:06d}": [cases.encode(pic(), "444", 90, restart_marker_rows=1) for _ in range(4)] + [cases.encode(pic(True))],
            f"{prefix}{start + 2:06d}": [cases.encode(pic(), "422"), cases.encode(pic(), "420", progressive=True), cases.encode(pic(), "420")]}


def _setup(tmp_path, prefix):
    from test_gpu_uap_e2e import GOLD, _checkpoints, _pca_pickle
    g = np.load(GOLD)
    root = str(tmp_path)
    videos = _videos(prefix, 600001)
    zips = os.path.join(root, "zips")
    _jpg_zips(zips, videos)
    ids = os.path.join(root, "ids.txt")
    with open(ids, "w") as f:
        f.write("\n".join(videos) + "\n")
    pca_path = os.path.join(root, "pca_model.pkl")
    _pca_pickle(g, pca_path)
    return root, zips, ids, _checkpoints(g, root), pca_path, videos


def test_extract_ref_feats_decode_hip_writes_the_same_file(tmp_path):
    """(--workers 0: the main process runs the loader's items itself; starting worker processes from a test process that has run
    the rest of the suite costs tens of seconds and is not what this test is about)"""
    import extract_ref_feats as E
    from test_gpu_frame_inputs import _npz, assert_same_npz
    root, zips, ids, models, _, videos = _setup(tmp_path, "R")
    _, arch, fmt, ckpt = models[1]
    out = {}
    for mode in ("host", "hip"):
        out[mode] = os.path.join(root, f"{arch}_{mode}")
        E.main(E.build_parser().parse_args(["--save_file", out[mode], "--zip_prefix", zips, "--input_file", ids, "--checkpoint_path", ckpt, "--arch", arch,
                                            "--weights_format", fmt, "--batch_size", "2", "--workers", "0", "--resize", "hip", "--decode", mode]))
    assert_same_npz(out["hip"] + ".npz", out["host"] + ".npz")
    assert len(_npz(out["hip"] + ".npz")["features"]) == sum(len(v) for v in videos.values())
    with pytest.raises(ValueError, match="resize"):
        E.main(E.build_parser().parse_args(["--save_file", out["hip"], "--zip_prefix", zips, "--input_file", ids, "--checkpoint_path", ckpt, "--arch", arch,
                                            "--weights_format", fmt, "--decode", "hip"]))


def test_extract_query_feats_decode_hip_writes_the_same_files(tmp_path):
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

    host, hip = run("host"), run("hip", "--decode", "hip")
    for key in keys:
        assert_same_npz(os.path.join(hip, key, "test_query.npz"), os.path.join(host, key, "test_query.npz"))
    assert_same_npz(os.path.join(hip, "test_query_sn.npz"), os.path.join(host, "test_query_sn.npz"))
    with pytest.raises(ValueError, match="resize"):
        E.main(E.build_parser().parse_args(["--split", "test", "--models"] + spec + ["--pca_model", pca_path, "--zip_prefix", zips, "--input_file", ids,
                                                                                      "--output_dir", os.path.join(root, "no"), "--decode", "hip"]))


def test_loader_and_decoder_hand_over_pillows_frames(dev, tmp_path):
    """ZipFrames(raw="bytes") -> HipDecode: two videos of a loader batch in one call, each video's device frames equal the
    worker's Pillow frames; the video with a progressive frame arrives decoded by the host"""
    from src.dataset import BytesVideo, ZipFrames, vit_transform_u8
    from src.image_preprocess import HipDecode
    videos = _videos("R", 700001)
    _jpg_zips(str(tmp_path), videos)
    t = vit_transform_u8(32, 32)
    packed, host = ZipFrames(list(videos), str(tmp_path), t, raw="bytes"), ZipFrames(list(videos), str(tmp_path), t, raw=True)
    items = [packed[i][0] for i in range(3)]
    assert isinstance(items[0], BytesVideo) and isinstance(items[1], BytesVideo) and isinstance(items[2], torch.Tensor)
    decoder = HipDecode(dev)
    for _ in range(2):                                            # the second call reuses the pinned buffer and the handle's tables
        frames = decoder(items[:2])
        torch.cuda.current_stream().synchronize()
        for i, f in enumerate(frames):
            assert f.is_cuda and torch.equal(f.cpu(), host[i][0]), i
    assert torch.equal(items[2], host[2][0])
