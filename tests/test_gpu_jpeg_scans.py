"""JPEG files of several scans decoded on the device (csrc/jpeg_scans.hip: vsc_jpeg_decode_scans_u8, ``--decode_scans hip``), through
the C ABI: every case of tests/jpeg_scans_cases.py in ONE call with the outputs at odd byte offsets between guard bands, against
Pillow bit for bit; a 70-frame call of baseline, progressive and one-scan-per-component frames whose single-scan frames equal
vsc_jpeg_decode_u8; the same call in several chunks; three calls on one handle and one on a fresh handle; the damaged files of
tests/jpeg_scans_cases.py, which passed the host sanitizers in tests/test_jpeg_scans_emulated.py (fixed files: nothing is fuzzed
on the device); and both entry points with ``--decode_scans hip`` against ``--decode host``, byte for byte."""
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

import jpeg_decode_cases as single  # noqa: E402
import jpeg_scans_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

P, I64 = ctypes.c_void_p, ctypes.c_int64


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


class Handle:
    def __init__(self, cap=0):
        from vsc_hip import _lib
        self.lib, self.h = _lib.load(), P()
        _lib.check(self.lib.vsc_jpeg_decode_create(None, ctypes.byref(self.h)))
        if cap:
            _lib.check(self.lib.vsc_jpeg_decode_scratch(self.h, cap, None, None))

    def chunks(self):
        from vsc_hip import _lib
        out = I64(-1)
        _lib.check(self.lib.vsc_jpeg_decode_scratch(self.h, 0, ctypes.byref(out), None))
        return out.value

    def close(self):
        self.lib.vsc_jpeg_decode_destroy(self.h)


def run_entry(file_list, dev, handle, guard=509, fill=0x5A, gap=5):
    """one vsc_jpeg_decode_scans_u8 call on the null stream: [guard | bytes | guard | output | guard | status | guard] in one arena,
    the frames packed from the output's start with ``gap`` bytes between them -> (rc, status, [frame], everything else intact)"""
    data, rows, srows, ptr, tables, out_len, outs = cases.call(file_list, 0, gap)
    n = len(rows)
    st_at = (3 * guard + len(data) + out_len + 3) & ~3
    arena = torch.full((st_at + 4 * n + guard,), 0xFF, dtype=torch.uint8, device=dev)
    d_at, o_at = guard, 2 * guard + len(data)
    arena[d_at:d_at + len(data)] = torch.from_numpy(data.copy()).to(dev)
    arena[o_at:o_at + out_len] = fill
    arena[st_at:st_at + 4 * n] = 0x77
    base = arena.data_ptr()
    rc = handle.lib.vsc_jpeg_decode_scans_u8(handle.h, P(base + d_at), len(data), rows.ctypes.data, n, srows.ctypes.data, ptr.ctypes.data, tables.ctypes.data, len(tables),
                                             P(base + o_at), out_len, P(base + st_at))
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    out = host[o_at:o_at + out_len]
    keep = np.ones(out_len, bool)
    for at, h, w in outs:
        keep[at:at + h * w * 3] = False
    intact = bool((host[:d_at] == 0xFF).all() and np.array_equal(host[d_at:d_at + len(data)], data) and (host[d_at + len(data):o_at] == 0xFF).all()
                  and (host[o_at + out_len:st_at] == 0xFF).all() and (host[st_at + 4 * n:] == 0xFF).all() and (out[keep] == fill).all())
    status = host[st_at:st_at + 4 * n].copy().view(np.int32)
    return rc, status, [out[at:at + h * w * 3].reshape(h, w, 3) for at, h, w in outs], intact


def test_every_case_in_one_call_equals_pillow(dev):
    names = cases.names()
    h = Handle()
    try:
        rc, status, frames, intact = run_entry([cases.file(n) for n in names], dev, h)
        assert rc == 0, h.lib.vsc_last_error()
        assert h.chunks() == 1
    finally:
        h.close()
    assert intact, "a guard band, a gap or the input was written"
    assert (status == 0).all(), [(n, int(s)) for n, s in zip(names, status) if s]
    bad = [(n, int((got != cases.pillow(n)).sum())) for n, got in zip(names, frames) if not np.array_equal(got, cases.pillow(n))]
    print(f"{len(names)} files in one call: {len(bad)} differ from Pillow {bad[:8]}")
    assert not bad, bad[:20]


@pytest.fixture(scope="module")
def mixed70():
    """70 frames, sizes 1 x 1 to 120 x 200: baseline (every third a restart interval), progressive, and one scan per component"""
    sizes = [(1, 1), (8, 8), (13, 17), (16, 16), (33, 47), (48, 64), (120, 200), (7, 2), (17, 9), (40, 56)]
    files, kinds = [], []
    for i in range(70):
        hh, ww = sizes[i % len(sizes)]
        s = ("420", "422", "444", "gray")[(i // 3) % 4]
        kind = ("baseline", "progressive", "per_component")[i % 3] if s != "gray" else ("baseline", "progressive")[i % 2]
        pic = single.picture(2000 + i, hh, ww)
        if kind == "baseline":
            files.append(cases.encode(pic, s, 75, **({"restart_marker_blocks": 3} if i % 9 == 0 else {})))
        elif kind == "progressive":
            files.append(cases.encode(pic, s, 85, progressive=True))
        else:
            files.append(cases.write_scans(single.encode(pic, s, 75)))
        kinds.append(kind)
    return files, kinds, [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]


def test_mixed_batch_and_single_scan_frames_equal_the_baseline_entry(dev, mixed70):
    from vsc_hip import ops
    files, kinds, want = mixed70
    assert set(kinds) == {"baseline", "progressive", "per_component"}
    h = Handle()
    try:
        rc, status, frames, intact = run_entry(files, dev, h)
    finally:
        h.close()
    assert rc == 0 and intact and (status == 0).all(), (rc, intact, status.tolist())
    for i, (got, ref) in enumerate(zip(frames, want)):
        assert np.array_equal(got, ref), (i, kinds[i], got.shape, int((got != ref).sum()))
    # the single-scan frames through vsc_jpeg_decode_u8 on the same rows
    base = [f for f, k in zip(files, kinds) if k == "baseline"]
    data, rows, tables, out_len, outs = single.call(base)
    out, st = ops.jpeg_decode(torch.from_numpy(data.copy()).to(dev), rows, tables, out_len)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert int(st.abs().sum()) == 0
    mine = [f for f, k in zip(frames, kinds) if k == "baseline"]
    for (at, hh, ww), got in zip(outs, mine):
        assert np.array_equal(out[at:at + hh * ww * 3].reshape(hh, ww, 3), got)


def test_chunked_scratch_gives_the_same_bytes(dev, mixed70):
    """a cap of 200 000 bytes: a 120 x 200 4:2:0 frame alone needs (128 * 208 + 2 * 64 * 104) * 3 = 119 808, so the 70 frames take several chunks"""
    files, kinds, want = mixed70
    h = Handle(cap=200000)
    try:
        rc, status, frames, intact = run_entry(files, dev, h, guard=512, gap=0)
        chunks = h.chunks()
    finally:
        h.close()
    assert rc == 0 and intact and (status == 0).all() and chunks >= 4, chunks
    assert all(np.array_equal(a, b) for a, b in zip(frames, want))


def test_three_calls_on_one_handle_and_a_fresh_handle_give_the_same_bytes(dev, mixed70):
    files, _, want = mixed70
    h = Handle()
    runs = []
    try:
        for _ in range(3):
            rc, status, frames, intact = run_entry(files, dev, h)
            assert rc == 0 and intact and (status == 0).all()
            runs.append(np.concatenate([f.reshape(-1) for f in frames]))
    finally:
        h.close()
    h = Handle()
    try:
        rc, status, frames, intact = run_entry(files, dev, h)
        assert rc == 0 and intact and (status == 0).all()
        runs.append(np.concatenate([f.reshape(-1) for f in frames]))
    finally:
        h.close()
    assert all(np.array_equal(runs[0], r) for r in runs[1:])
    assert np.array_equal(runs[0], np.concatenate([w.reshape(-1) for w in want]))


def test_damaged_files_set_their_status_only(dev):
    """the pre-built damaged files between two good ones, all in one call"""
    good = ["33x47_420_q75_noise", "16x16_gray_q30_ramp"]
    damaged = cases.damaged()
    files, expect, names = [cases.file(good[0])], [0], [good[0]]
    for k, name in enumerate(sorted(damaged)):
        files += [damaged[name][0], cases.file(good[(k + 1) % 2])]
        expect += [damaged[name][1], 0]
        names += [None, good[(k + 1) % 2]]
    h = Handle()
    try:
        rc, status, frames, intact = run_entry(files, dev, h)
    finally:
        h.close()
    assert rc == 0 and intact, "a guard band, a gap or the input was written"
    assert status.tolist() == expect and all(e != 0 for e in expect[1::2]), (status.tolist(), expect)
    for i, got in enumerate(frames):
        if names[i] is not None:
            assert np.array_equal(got, cases.pillow(names[i])), i


def test_ops_and_refusals(dev):
    from vsc_hip import _lib, ops
    files = [cases.file("13x17_420_q75_noise"), single.files("8x8_444")[0]]
    data, rows, srows, ptr, tables, out_len, outs = cases.call(files)
    dd = torch.from_numpy(data.copy()).to(dev)
    out, status = ops.jpeg_decode(dd, rows, tables, out_len, scans=(srows, ptr))
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    out = out.cpu().numpy()
    assert np.array_equal(out[:13 * 17 * 3].reshape(13, 17, 3), cases.pillow("13x17_420_q75_noise"))
    assert np.array_equal(out[13 * 17 * 3:].reshape(8, 8, 3), single.pillow("8x8_444")[0])
    keep = torch.full((out_len,), 0x5A, dtype=torch.uint8, device=dev)
    swapped = srows.copy()
    swapped[[0, 1]] = swapped[[1, 0]]                       # AC before DC: refused before anything is launched
    with pytest.raises(_lib.VscHipError, match="before its first DC scan"):
        ops.jpeg_decode(dd, rows, tables, out_len, out=keep, scans=(swapped, ptr))
    with pytest.raises(_lib.VscHipError, match="leave coefficient"):
        ops.jpeg_decode(dd, rows[:1], tables, out_len, out=keep, scans=(srows[:9], np.asarray([0, 9], np.int64)))
    with pytest.raises(ValueError, match="several scans"):
        ops.jpeg_decode(dd, rows, tables, out_len, out=keep, scans=(srows, ptr), split="all")
    torch.cuda.synchronize()
    assert bool((keep == 0x5A).all())


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
def _videos(prefix, start):
    """three videos of 48 x 64 frames: all baseline, all progressive, mixed (progressive, one scan per component, table ids 2 and 3)"""
    rng = np.random.default_rng(start)
    pic = lambda gray=False: single.picture(int(rng.integers(1 << 30)), 48, 64, gray=gray)     # noqa: E731
    return {f"{prefix}{start:06d}": [single.encode(pic(), "420") for _ in range(4)],
            f"{prefix}{start + 1:06d}": [single.encode(pic(), s, 80, progressive=True) for s in ("420", "444", "422")] + [single.encode(pic(True), progressive=True)],
            f"{prefix}{start + 2:06d}": [single.encode(pic(), "422"), single.encode(pic(), "420", progressive=True), cases.write_scans(single.encode(pic(), "420")),
                                         cases.table_ids_2_3(single.encode(pic(), "444"))]}


def _setup(tmp_path, prefix):
    from test_gpu_jpeg_decode import _jpg_zips
    from test_gpu_uap_e2e import GOLD, _checkpoints, _pca_pickle
    g = np.load(GOLD)
    root = str(tmp_path)
    videos = _videos(prefix, 800001)
    zips = os.path.join(root, "zips")
    _jpg_zips(zips, videos)
    ids = os.path.join(root, "ids.txt")
    with open(ids, "w") as f:
        f.write("\n".join(videos) + "\n")
    pca_path = os.path.join(root, "pca_model.pkl")
    _pca_pickle(g, pca_path)
    return root, zips, ids, _checkpoints(g, root), pca_path, videos


def test_loader_routing(dev, tmp_path):
    """with decode_scans="hip" no video is decoded by the loader; with "host" the routing is today's: the two videos that hold a
    progressive frame arrive decoded by the host"""
    from src.dataset import BytesVideo, ZipFrames, check_decode_scans, vit_transform_u8
    from src.image_preprocess import HipDecode
    from test_gpu_jpeg_decode import _jpg_zips
    videos = _videos("R", 810001)
    _jpg_zips(str(tmp_path), videos)
    t = vit_transform_u8(32, 32)
    host = ZipFrames(list(videos), str(tmp_path), t, raw=True)
    today = ZipFrames(list(videos), str(tmp_path), t, raw="bytes")
    items = [today[i][0] for i in range(3)]
    assert isinstance(items[0], BytesVideo) and isinstance(items[1], torch.Tensor) and isinstance(items[2], torch.Tensor) and today.host_decoded == 2
    packed = ZipFrames(list(videos), str(tmp_path), t, raw="bytes", decode_scans="hip")
    items = [packed[i][0] for i in range(3)]
    assert all(isinstance(v, BytesVideo) for v in items) and packed.host_decoded == 0
    for split in ("none", "all"):
        decoder = HipDecode(dev, split, "hip")
        frames = decoder(items)
        torch.cuda.current_stream().synchronize()
        for i, f in enumerate(frames):
            assert f.is_cuda and torch.equal(f.cpu(), host[i][0]), (split, i)
    with pytest.raises(ValueError, match="decode='hip'"):
        check_decode_scans("hip", "host")
    with pytest.raises(ValueError, match="decode_scans must be one of"):
        check_decode_scans("device")
    with pytest.raises(ValueError, match="decode='hip'"):
        ZipFrames(list(videos), str(tmp_path), t, raw=True, decode_scans="hip")


def test_extract_ref_feats_decode_scans_hip_writes_the_same_file(tmp_path):
    import extract_ref_feats as E
    from test_gpu_frame_inputs import _npz, assert_same_npz
    root, zips, ids, models, _, videos = _setup(tmp_path, "R")
    _, arch, fmt, ckpt = models[1]
    out = {}
    for name, extra in (("host", ["--decode", "host"]), ("hip", ["--decode", "hip", "--decode_scans", "hip"]),
                        ("split", ["--decode", "hip", "--decode_scans", "hip", "--decode_split", "all"])):
        out[name] = os.path.join(root, f"{arch}_{name}")
        E.main(E.build_parser().parse_args(["--save_file", out[name], "--zip_prefix", zips, "--input_file", ids, "--checkpoint_path", ckpt, "--arch", arch,
                                            "--weights_format", fmt, "--batch_size", "2", "--workers", "0", "--resize", "hip", *extra]))
    for name in ("hip", "split"):
        assert_same_npz(out[name] + ".npz", out["host"] + ".npz")
    assert len(_npz(out["hip"] + ".npz")["features"]) == sum(len(v) for v in videos.values())
    with pytest.raises(ValueError, match="decode='hip'"):
        E.main(E.build_parser().parse_args(["--save_file", out["hip"], "--zip_prefix", zips, "--input_file", ids, "--checkpoint_path", ckpt, "--arch", arch,
                                            "--weights_format", fmt, "--resize", "hip", "--decode_scans", "hip"]))


def test_extract_query_feats_decode_scans_hip_writes_the_same_files(tmp_path):
    import extract_query_feats as E
    from test_gpu_frame_inputs import assert_same_npz
    root, zips, ids, models, pca_path, videos = _setup(tmp_path, "Q")
    spec = [f"{arch}:{fmt}:{ckpt}" for _, arch, fmt, ckpt in models]
    keys = [os.path.split(ckpt)[-1].split(".")[0] for _, _, _, ckpt in models]

    def run(name, *extra):
        out = os.path.join(root, name)
        E.main(E.build_parser().parse_args(["--split", "test", "--models"] + spec + ["--pca_model", pca_path, "--zip_prefix", zips, "--input_file", ids,
                                                                                      "--output_dir", out, "--workers", "0", "--resize", "hip", *extra]))
        return out

    host, hip = run("host", "--decode", "host"), run("hip", "--decode", "hip", "--decode_scans", "hip")
    for key in keys:
        assert_same_npz(os.path.join(hip, key, "test_query.npz"), os.path.join(host, key, "test_query.npz"))
    assert_same_npz(os.path.join(hip, "test_query_sn.npz"), os.path.join(host, "test_query_sn.npz"))
    # the loader: no video decoded by a worker with the option, today's routing without it
    on = E.QueryVideos(list(videos), zips, [224], resize="hip", decode="hip", decode_scans="hip")
    off = E.QueryVideos(list(videos), zips, [224], resize="hip", decode="hip")
    for i in range(3):
        on[i], off[i]
    assert on.host_decoded == 0 and off.host_decoded == 2
    with pytest.raises(ValueError, match="decode='hip'"):
        E.main(E.build_parser().parse_args(["--split", "test", "--models"] + spec + ["--pca_model", pca_path, "--zip_prefix", zips, "--input_file", ids,
                                                                                      "--output_dir", os.path.join(root, "no"), "--resize", "hip", "--decode_scans", "hip"]))
