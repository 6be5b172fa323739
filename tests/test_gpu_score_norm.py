"""Score normalisation on the device (csrc/score_norm.hip; vsc.baseline.score_normalization, device="hip"; --score_norm hip):
everything it writes is compared with the default host path BIT FOR BIT -- uint32 views, no tolerance anywhere.

  kernels      vsc_column_var_f32 against numpy's x.var(axis=0); vsc_score_norm_rows_f32 against np.delete -> ops.l2_normalize_ (on this
               device) -> np.concatenate; vsc_score_norm_bias_f32 against numpy's -beta * sims[:, :nk].mean(axis=1).  Outputs stand
               between NaN guard bands and inside padded rows, all of which must survive.
  functions    score_normalize / query_score_normalize / ref_score_normalize / low_variance_dim, device="hip" against device="host"
  entry points concat_pca_sn.main and sscd_baseline.main with --score_norm hip write the files of the default run
  placement    the same call three times; every entry on a side stream behind a spinning wave with decoy operands before and after
"""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import score_norm_cases as cases  # noqa: E402
import score_norm_contract as C  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 1024                      # NaN floats before and behind every output
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def guarded(n, width, ld, dev):
    """-> (raw, body [n, ld], out = body[:, :width]): NaN everywhere; the kernel may write `out` only"""
    raw = torch.full((2 * GUARD + max(n, 1) * ld,), NAN, dtype=torch.float32, device=dev)
    body = raw[GUARD:GUARD + max(n, 1) * ld].view(max(n, 1), ld)[:n]
    return raw, body, body[:, :width]


def assert_untouched(raw, body, width):
    assert bool(torch.isnan(raw[:GUARD]).all()) and bool(torch.isnan(raw[raw.numel() - GUARD:]).all()), "a guard band changed"
    assert bool(torch.isnan(body[:, width:]).all()), "row padding changed"


def dev_bits(t):
    return C.bits(t.detach().cpu().contiguous().numpy())


# ---- vsc_column_var_f32 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,ld", cases.VAR_SHAPES + [cases.VAR_SHAPE_LARGE])
def test_column_var_is_numpys(dev, n, d, ld):
    from vsc_hip import _lib, ops
    x = cases.offset_rows(n, d, ld)
    want = np.ascontiguousarray(x[:, :d]).var(axis=0)
    xd = torch.from_numpy(x).to(dev)
    got = ops.column_var(xd[:, :d])
    assert got.shape == (d,) and np.array_equal(dev_bits(got), C.bits(want)), np.nonzero(dev_bits(got) != C.bits(want))[0][:10]
    # into a guarded buffer, three times: the same bytes, nothing else written, the NaN padding of x never read
    raw = torch.full((2 * GUARD + d,), NAN, dtype=torch.float32, device=dev)
    out = raw[GUARD:GUARD + d]
    lib = _lib.load()
    for _ in range(3):
        out.fill_(NAN)
        _lib.check(lib.vsc_column_var_f32(ops.score_norm_handle(), ctypes.c_void_p(xd.data_ptr()), n, d, ld, ctypes.c_void_p(out.data_ptr())))
        assert np.array_equal(dev_bits(out), C.bits(want))
    assert bool(torch.isnan(raw[:GUARD]).all()) and bool(torch.isnan(raw[GUARD + d:]).all())


def test_column_var_ties_take_the_first_and_bad_calls_are_refused(dev):
    from vsc_hip import _lib, ops
    x = cases.offset_rows(200, 70)
    x[:, 66] = x[:, 3]
    x[:, [3, 66]] *= np.float32(1e-3)
    var = ops.column_var(torch.from_numpy(x).to(dev)).cpu().numpy()
    assert C.bits(var)[3] == C.bits(var)[66] and int(np.argmin(var)) == 3 == int(x.var(axis=0).argmin())
    lib, h, xd, out = _lib.load(), ops.score_norm_handle(), torch.from_numpy(x).to(dev), torch.zeros(70, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.vsc_column_var_f32(h, p(xd), 0, 70, 70, p(out)) != 0
    assert lib.vsc_column_var_f32(h, p(xd), 200, 0, 70, p(out)) != 0
    assert lib.vsc_column_var_f32(h, p(xd), 200, 70, 69, p(out)) != 0
    assert lib.vsc_column_var_f32(h, None, 200, 70, 70, p(out)) != 0
    assert lib.vsc_column_var_f32(None, p(xd), 200, 70, 70, p(out)) != 0                        # no handle
    with pytest.raises(ValueError):
        ops.column_var(xd[:0])


# ---- vsc_score_norm_rows_f32 -------------------------------------------------------------------------------------------------------
def host_chain(x, drop, normalize, append, last, dev):
    """today's chain: np.delete, vsc_l2_normalize_f32 on the narrowed contiguous rows (on this device), np.concatenate"""
    from vsc_hip import ops
    body = np.ascontiguousarray(np.delete(x, drop, axis=1) if drop >= 0 else x)
    if normalize and len(body):
        body = ops.l2_normalize_(torch.from_numpy(body).to(dev)).cpu().numpy()
    if append == 0:
        return body
    return np.concatenate([body, np.ones_like(body[:, :1]) if append == 1 else last[:, None]], axis=1)


@pytest.mark.parametrize("d", cases.ROWS_D)
def test_rows_equal_delete_normalize_concatenate(dev, d):
    from vsc_hip import ops
    ldx = d + 3
    x = cases.descriptor_rows(d, ldx)
    n = len(x)
    last = (np.arange(n, dtype=np.float32) * np.float32(-0.37) - np.float32(100.0)).astype(np.float32)
    xd, lastd = torch.from_numpy(x).to(dev), torch.from_numpy(last).to(dev)
    for drop in cases.drops(d):
        for append in (0, 1, 2):
            for normalize in (0, 1):
                width = d - (drop >= 0) + (append != 0)
                raw, body, out = guarded(n, width, width + 5, dev)
                got = ops.score_norm_rows(xd[:, :d], drop, bool(normalize), append, last=lastd, out=out)
                want = host_chain(x[:, :d], drop, normalize, append, last, dev)
                assert np.array_equal(dev_bits(got), C.bits(want)), (d, drop, append, normalize)
                assert_untouched(raw, body, width)
                keep = [c for c in range(d) if c != drop]
                for r in (2, 4):                                     # the zero row; the row of 1e-30, whose squares underflow
                    assert np.array_equal(dev_bits(got[r, :len(keep)]), C.bits(x[r, keep])), (d, drop, r)
    assert bool(torch.isnan(xd[:, d:]).all())                        # x itself: untouched
    assert np.array_equal(dev_bits(xd[:, :d]), C.bits(np.ascontiguousarray(x[:, :d])))
    # and the contract's own statement of the normalisation agrees with the device
    assert np.array_equal(C.bits(C.rows(x[:, :d], min(1, d - 1), True, 1)), C.bits(host_chain(x[:, :d], min(1, d - 1), 1, 1, last, dev)))


def test_rows_empty_and_refused_calls(dev):
    from vsc_hip import _lib, ops
    from vsc_hip._lib import VscHipError
    x = torch.from_numpy(np.ascontiguousarray(cases.descriptor_rows(8, 8))).to(dev)
    assert tuple(ops.score_norm_rows(x[:0], 3, True, 1).shape) == (0, 8)         # n = 0: nothing launched
    big = torch.zeros(6 * 8 + 6 * 9, dtype=torch.float32, device=dev)
    xin = big[:48].view(6, 8)
    xin.copy_(x)
    with pytest.raises(VscHipError, match="overlaps"):
        ops.score_norm_rows(xin, 0, True, 1, out=xin)                            # in place
    with pytest.raises(VscHipError, match="overlaps"):
        ops.score_norm_rows(xin, 0, True, 0, out=big[8:8 + 42].view(6, 7))       # shifted into x
    adjacent = ops.score_norm_rows(xin, 0, True, 0, out=big[48:48 + 42].view(6, 7))
    assert np.array_equal(dev_bits(adjacent), dev_bits(ops.score_norm_rows(x, 0, True, 0)))
    lib, h, p = _lib.load(), ops.score_norm_handle(), lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.zeros((6, 9), dtype=torch.float32, device=dev)
    assert lib.vsc_score_norm_rows_f32(h, p(x), 6, 8, 8, 8, 1, 0, None, p(out), 9) != 0      # drop == d
    assert lib.vsc_score_norm_rows_f32(h, p(x), 6, 8, 8, 0, 2, 0, None, p(out), 9) != 0      # normalize
    assert lib.vsc_score_norm_rows_f32(h, p(x), 6, 8, 8, 0, 1, 3, None, p(out), 9) != 0      # append
    assert lib.vsc_score_norm_rows_f32(h, p(x), 6, 8, 8, 0, 1, 2, None, p(out), 9) != 0      # append = 2 without its column
    assert lib.vsc_score_norm_rows_f32(h, p(x), 6, 8, 7, 0, 1, 0, None, p(out), 9) != 0      # ldx < d
    assert lib.vsc_score_norm_rows_f32(h, p(x), 6, 8, 8, -1, 1, 1, None, p(out), 8) != 0     # ldo < width
    torch.cuda.synchronize()


# ---- vsc_score_norm_bias_f32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", cases.NKS)
def test_bias_is_numpys(dev, nk):
    from vsc_hip import ops
    nq, ldk = 300, nk + 3
    topk, gate = cases.topk_scores(nq, nk, ldk)
    td, gd = torch.from_numpy(topk).to(dev), torch.from_numpy(gate).to(dev)
    for beta in (1.2, 1.5):
        want = -beta * np.ascontiguousarray(topk[:, :nk]).mean(axis=1)
        got = ops.score_norm_bias(td, nk, beta)
        assert np.array_equal(dev_bits(got), C.bits(want)), (nk, beta)
        gated = ops.score_norm_bias(td, nk, beta, gd).cpu().numpy()
        assert np.array_equal(C.bits(gated), C.bits(np.where(gate != 0, np.float32(-100.0), want)))
        dense = ops.score_norm_bias(td[:, :nk].contiguous(), nk, beta)
        assert np.array_equal(dev_bits(dense), C.bits(want))


def test_bias_guards_and_refusals(dev):
    from vsc_hip import _lib, ops
    topk, gate = cases.topk_scores(70, 129, 130)
    td = torch.from_numpy(topk).to(dev)
    raw = torch.full((2 * GUARD + 70,), NAN, dtype=torch.float32, device=dev)
    out = raw[GUARD:GUARD + 70]
    lib, h, p = _lib.load(), ops.score_norm_handle(), lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.vsc_score_norm_bias_f32(h, p(td), 70, 130, 129, -1.0, None, p(out)) != 0      # numpy's sum recurses beyond 128
    assert lib.vsc_score_norm_bias_f32(h, p(td), 70, 130, 0, -1.0, None, p(out)) != 0
    assert lib.vsc_score_norm_bias_f32(h, p(td), 70, 7, 8, -1.0, None, p(out)) != 0          # ldk < nk
    assert lib.vsc_score_norm_bias_f32(h, None, 0, 130, 8, -1.0, None, None) == 0            # nq = 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(raw).all())                                                         # a refused call writes nothing
    _lib.check(lib.vsc_score_norm_bias_f32(h, p(td), 70, 130, 128, -1.0, None, p(out)))
    torch.cuda.synchronize()
    assert np.array_equal(dev_bits(out), C.bits(-1.0 * np.ascontiguousarray(topk[:, :128]).mean(axis=1)))
    assert bool(torch.isnan(raw[:GUARD]).all()) and bool(torch.isnan(raw[GUARD + 70:]).all())


def test_the_same_call_three_times_gives_the_same_bytes(dev):
    from vsc_hip import ops
    x = torch.from_numpy(np.ascontiguousarray(cases.offset_rows(1000, 513))).to(dev)
    topk = torch.from_numpy(cases.topk_scores(1000, 17, 20)[0]).to(dev)
    for call in (lambda: ops.column_var(x), lambda: ops.score_norm_rows(x, 64, True, 1), lambda: ops.score_norm_bias(topk, 17, 1.2)):
        first = dev_bits(call())
        assert np.array_equal(first, dev_bits(call())) and np.array_equal(first, dev_bits(call()))


# ---- the three functions -------------------------------------------------------------------------------------------------------------
def video_set(prefix, lens, d, seed):
    """videos as `load_features` hands them out: consecutive row views of one float32 array; descriptors with a different spread in
    every dimension, so the low-variance dimension is a definite one"""
    from vsc.index import VideoFeature
    rs = np.random.RandomState(seed)
    spread = rs.uniform(0.5, 1.5, d)
    spread[d // 3] = 0.2
    base = (rs.standard_normal((sum(lens), d)) * spread + rs.uniform(-0.3, 0.3, d)).astype(np.float32)
    out, lo = [], 0
    for i, n in enumerate(lens):
        out.append(VideoFeature(video_id=f"{prefix}{i:06d}", timestamps=np.arange(n, dtype=np.float32) + np.float32(i), feature=base[lo:lo + n]))
        lo += n
    return out


def assert_same_videos(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.video_id == b.video_id and np.array_equal(a.timestamps, b.timestamps)
        assert a.feature.shape == b.feature.shape and a.feature.dtype == b.feature.dtype == np.float32, (a.video_id, a.feature.shape, b.feature.shape)
        assert np.array_equal(C.bits(a.feature), C.bits(b.feature)), a.video_id


_sets = {}


def sets_for(d):
    if d not in _sets:
        rs = np.random.RandomState(d)
        q_lens = rs.randint(0, 61, 40)
        q_lens[5] = 0                                                # one video without rows
        r_lens = rs.randint(1, 61, 40)
        queries, refs = video_set("Q", q_lens.tolist(), d, 1), video_set("R1", r_lens.tolist(), d, 2)
        noise = video_set("R2", rs.randint(1, 61, 30).tolist(), d, 3)
        scores = {q.video_id: 1.0 for q in queries}
        scores[queries[3].video_id] = 0.0001                         # two videos below the threshold: bias -100
        scores[queries[17].video_id] = 0.0
        _sets[d] = (queries, refs, noise, scores)
    return _sets[d]


@pytest.mark.parametrize("d,nk,beta", [(32, 1, 1.2), (512, 10, 1.5)])
def test_functions_on_the_device_equal_the_host_path(dev, d, nk, beta):
    from vsc.baseline import score_normalization as sn
    queries, refs, noise, scores = sets_for(d)
    dim = sn.low_variance_dim(noise)
    assert dim == d // 3
    bank = sn.ScoreNormBank(noise)
    assert sn.low_variance_dim(noise, device="hip") == dim == sn.low_variance_dim(bank, device="hip") == bank.low_variance_dim()
    from src import matching
    assert matching.calclualte_low_var_dim(bank, device="hip") == dim == matching.calclualte_low_var_dim(noise)

    want = sn.query_score_normalize(queries, noise, scores, 0.001, dim, beta=beta, nk=nk)
    for norm in (noise, bank):                                       # the set as a list and as the handle
        got = sn.query_score_normalize(queries, norm, scores, 0.001, dim, beta=beta, nk=nk, device="hip")
        assert_same_videos(got, want)
        assert got[5].feature.shape == (0, d) and (got[3].feature[:, -1] == np.float32(-100.0)).all() and (got[17].feature[:, -1] == np.float32(-100.0)).all()
        assert np.array_equal(dev_bits(got.rows_dev), C.bits(np.concatenate([v.feature for v in want])))
    want = sn.ref_score_normalize(refs, noise, beta=beta, nk=nk)
    for norm in (noise, bank):
        assert_same_videos(sn.ref_score_normalize(refs, norm, beta=beta, nk=nk, device="hip"), want)
    assert_same_videos(sn.ref_score_normalize(sn.ScoreNormBank(refs), bank, beta=beta, nk=nk, device="hip"), want)
    want_q, want_r = sn.score_normalize(queries, refs, noise, beta=beta, nk=nk)
    for norm in (noise, bank):
        got_q, got_r = sn.score_normalize(queries, refs, norm, beta=beta, nk=nk, device="hip")
        assert_same_videos(got_q, want_q)
        assert_same_videos(got_r, want_r)
    # the two flags map to the kernel's
    for kw in ({"l2_normalize": False}, {"replace_dim": False}, {"l2_normalize": False, "replace_dim": False}):
        want_q, want_r = sn.score_normalize(queries, refs, noise, beta=beta, nk=nk, **kw)
        got_q, got_r = sn.score_normalize(queries, refs, bank, beta=beta, nk=nk, device="hip", **kw)
        assert_same_videos(got_q, want_q)
        assert_same_videos(got_r, want_r)
        assert got_r[0].feature.shape[1] == d + (not kw.get("replace_dim", True))
        assert_same_videos(sn.query_score_normalize(queries, bank, scores, 0.001, dim, beta=beta, nk=nk, device="hip", **kw),
                           sn.query_score_normalize(queries, noise, scores, 0.001, dim, beta=beta, nk=nk, **kw))
    # videos that are not views of one array (here: copies in another order) take the one concatenation instead
    shuffled = [dataclasses.replace(v, feature=v.feature.copy()) for v in reversed(refs)]
    assert_same_videos(sn.ref_score_normalize(shuffled, bank, beta=beta, nk=nk, device="hip"), sn.ref_score_normalize(shuffled, noise, beta=beta, nk=nk))
    with pytest.raises(ValueError, match="ScoreNormBank"):
        sn.ref_score_normalize(refs, bank)                           # the handle is device memory: device="hip" only
    with pytest.raises(Exception, match="against VSC rules"):
        sn.ref_score_normalize(noise, bank, device="hip")


# ---- entry points ----------------------------------------------------------------------------------------------------------------------
def npz_arrays(path):
    with np.load(path, allow_pickle=False) as data:
        return {k: data[k] for k in data.files}


def assert_same_npz(a, b):
    assert sorted(a) == sorted(b) == ["features", "timestamps", "video_ids"]
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_concat_pca_sn_writes_the_same_files(dev, tmp_path):
    import concat_pca_sn as entry
    from tools import synth
    from vsc.index import VideoFeature
    from vsc.storage import store_features
    models, dims = ["m_a", "m_b"], [24, 40]
    vids = {"train_refs": [f"R1{i:05d}" for i in range(5)], "test_refs": [f"R2{i:05d}" for i in range(4)]}
    for mi, (m, d) in enumerate(zip(models, dims)):
        os.makedirs(tmp_path / m)
        for si, (name, ids) in enumerate(vids.items()):
            store_features(str(tmp_path / m / f"{name}.npz"),
                           [VideoFeature(video_id=v, timestamps=np.arange(6 + vi, dtype=np.float64),
                                         feature=synth.normalish(1000 * mi + 100 * si + vi, (6 + vi, d)) * (1 + vi)) for vi, v in enumerate(ids)])
    base = ["--root", str(tmp_path), "--models", *models, "--pca_model", str(tmp_path / "pca.npz"), "--dim", "16"]
    entry.main(entry.build_parser().parse_args(base + ["--fit_pca", "--pca_fit", "hip"]))
    default = {name: npz_arrays(tmp_path / f"{name}_sn.npz") for name in vids}
    for name in vids:
        os.remove(tmp_path / f"{name}_sn.npz")
    entry.main(entry.build_parser().parse_args(base + ["--score_norm", "hip"]))
    for name in vids:
        assert_same_npz(npz_arrays(tmp_path / f"{name}_sn.npz"), default[name])
        assert default[name]["features"].shape[1] == 16
    ns = entry.build_parser().parse_args(base)
    del ns.score_norm                                                # a namespace from before the option: the host path
    entry.main(ns)
    for name in vids:
        assert_same_npz(npz_arrays(tmp_path / f"{name}_sn.npz"), default[name])


def test_sscd_baseline_writes_the_same_files_and_searches_the_adopted_rows(dev, tmp_path, monkeypatch):
    import vsc.baseline.sscd_baseline as entry
    from tools import synth
    from vsc.index import FlatIPBank, VideoFeature
    from vsc.storage import store_features
    d = 64
    refs = [VideoFeature(f"R{i:06d}", np.arange(30.0), synth.descriptor_bank(300 + i, 30, d)) for i in range(12)]
    noise = [VideoFeature(f"R{100 + i:06d}", np.arange(25.0), synth.descriptor_bank(900 + i, 25, d)) for i in range(10)]
    queries = []
    for i in range(8):
        f = synth.descriptor_bank(600 + i, 20, d)
        f[3:15] = refs[i].feature[5:17]                              # every query copies a run of one reference
        queries.append(VideoFeature(f"Q{i:06d}", np.arange(20.0), f))
    n_ref_rows = sum(len(r) for r in refs)
    for name, videos in (("q", queries), ("r", refs), ("n", noise)):
        store_features(tmp_path / f"{name}.npz", videos)
    base = ["--query_features", str(tmp_path / "q.npz"), "--ref_features", str(tmp_path / "r.npz"), "--score_norm_features",
            str(tmp_path / "n.npz"), "--overwrite", "--alignment", "hip"]
    entry.main(entry.build_parser().parse_args(base + ["--output_path", str(tmp_path / "host")]))

    uploads, adopted = [], []
    to_device, adopt = FlatIPBank._to_device, FlatIPBank.adopt_device_rows
    monkeypatch.setattr(FlatIPBank, "_to_device", staticmethod(lambda host: (uploads.append(tuple(host.shape)), to_device(host))[1]))
    monkeypatch.setattr(FlatIPBank, "adopt_device_rows", lambda self, rows: (adopted.append(tuple(rows.shape)), adopt(self, rows))[1])
    entry.main(entry.build_parser().parse_args(base + ["--output_path", str(tmp_path / "hip"), "--score_norm", "hip", "--candidates", "hip"]))
    assert adopted == [(n_ref_rows, d)], adopted                     # the index took the normalised references as they stood on the device
    assert uploads and not [s for s in uploads if len(s) == 2 and s[0] == n_ref_rows], uploads   # ... and uploaded no bank
    for name in ("sn_queries.npz", "sn_refs.npz"):
        assert_same_npz(npz_arrays(tmp_path / "hip" / name), npz_arrays(tmp_path / "host" / name))
    for name in ("candidates.csv", "matches.csv"):
        assert (tmp_path / "hip" / name).read_bytes() == (tmp_path / "host" / name).read_bytes(), name
    assert len((tmp_path / "host" / "candidates.csv").read_text().splitlines()) > 8


# ---- stream order -----------------------------------------------------------------------------------------------------------------------
def spin_ticks_for(ms, dev):
    """ticks of vsc_debug_spin_ticks that last `ms`: the rate from two spins of different lengths (the launch cost cancels)"""
    from vsc_hip import _lib
    lib, out = _lib.load(), torch.zeros(1, dtype=torch.int64, device=dev)

    def spin_ms(ticks):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        _lib.check(lib.vsc_debug_spin_ticks(ticks, ctypes.c_void_p(out.data_ptr()), None))
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    spin_ms(1000)
    a, b = min(spin_ms(200_000) for _ in range(3)), min(spin_ms(2_000_000) for _ in range(3))
    assert b > a
    return int(ms * 1_800_000 / (b - a))


@pytest.mark.parametrize("entry", ["column_var", "rows", "bias"])
def test_entries_only_enqueue_on_the_callers_stream(dev, entry):
    """Behind a wave that spins for 40 ms on a side stream: the operands hold a decoy until copies ON THAT STREAM replace them, the
    call follows, the result is copied away on that stream and the operands are overwritten with the decoy again.  A kernel issued on
    any other stream, or a call that waited for the device, would read the decoy or return late."""
    from vsc_hip import _lib, ops
    lib = _lib.load()
    rs = np.random.RandomState(11)
    if entry == "column_var":
        real = cases.offset_rows(300, 70)
        call = lambda x: ops.column_var(x)
        want = lambda: real.var(axis=0)
    elif entry == "rows":
        real = np.ascontiguousarray(cases.offset_rows(300, 70))
        call = lambda x: ops.score_norm_rows(x, 7, True, 1)
        want = lambda: host_chain(real, 7, 1, 1, None, dev)
    else:
        real = np.ascontiguousarray(cases.topk_scores(300, 10, 10)[0])
        call = lambda x: ops.score_norm_bias(x, 10, 1.5)
        want = lambda: -1.5 * real.mean(axis=1)
    expected = want()
    decoy = torch.from_numpy(rs.standard_normal(real.shape).astype(np.float32)).to(dev)
    staged = torch.from_numpy(real).to(dev)
    operand = decoy.clone()
    spin_out = torch.zeros(1, dtype=torch.int64, device=dev)
    ticks = spin_ticks_for(40.0, dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    started = torch.cuda.Event()
    _lib.check(lib.vsc_debug_spin_ticks(ticks, ctypes.c_void_p(spin_out.data_ptr()), ctypes.c_void_p(side.cuda_stream)))
    started.record(side)
    with torch.cuda.stream(side):
        operand.copy_(staged, non_blocking=True)
        out = call(operand)
        returned_in_time = not started.query()
        kept = out.clone()
        operand.copy_(decoy, non_blocking=True)
    side.synchronize()
    torch.cuda.synchronize()
    assert returned_in_time, "the call returned only after the delay had ended: it must only enqueue"
    assert np.array_equal(dev_bits(kept), C.bits(np.asarray(expected, np.float32))), entry
