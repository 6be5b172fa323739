"""The exact L2 search on the device (csrc/l2_search.hip) against its contract (tests/l2_search_contract.py): distances as uint32
bits, ids equal -- on every path, and with the demand that the certified fast path is the one that ran where the reference
arithmetic says it can (tests/test_l2_search_cpu.py::test_certificate_rule_on_the_reference_arithmetic)."""
import ctypes

import numpy as np
import pytest
import torch

import l2_search_contract as C

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    _lib.load().vsc_search_release_scratch()


def _ops():
    from vsc_hip import _lib, ops
    return _lib, ops


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.uint32)


def _knn(q, r, k, dev, path=None, offset=0, bank=False):
    _lib, ops = _ops()
    qd, rd = _t(q, dev), _t(r, dev)
    b = None
    if bank:
        aug, _, mx = ops.l2_augment(rd)
        b = (aug, mx)
    with _lib.option("VSC_L2_PATH", path):
        D, I = ops.knn_l2(qd, rd, k, offset, bank=b)
        D, I = D.cpu().numpy(), I.cpu().numpy()
    return D, I, ops.knn_l2_last_path()


def _same(got, want):
    return np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])


_data = {}


def _case(nq, nr, d, k):
    """inputs, the contract's result, and whether the reference arithmetic certifies every row (the CPU test asserts those)"""
    key = (nq, nr, d, k)
    if key not in _data:
        if (nq, nr, d) == (17, 500, 24):
            q, r = C.flat_l2_data()
            sure = True
        elif (nr, d) in ((3000, 512), (5000, 33)):
            q, r = (C.unit(11, nq, d), C.unit(12, nr, d)) if d == 512 else (C.unit(13, nq, d), C.unit(14, nr, d))
            sure = True
        else:
            rng = np.random.RandomState(nq * 1000 + d)
            q, r = (rng.randn(nq, d) * 3).astype(np.float32), (rng.randn(nr, d) * 3).astype(np.float32)
            sure = False
        _data[key] = (q, r, C.knn(q, r, k), sure)
    return _data[key]


CASES = [(1, 1, 1, 1), (3, 70, 4, 5), (17, 500, 24, 9), (16, 3000, 512, 10), (16, 3000, 512, 100), (5, 1500, 33, 1024), (9, 600, 513, 7),
         (16, 5000, 33, 10)]


@pytest.mark.parametrize("nq,nr,d,k", CASES)
def test_bits_equal_the_contract_on_every_path(dev, nq, nr, d, k):
    q, r, want, sure = _case(nq, nr, d, k)
    auto = _knn(q, r, k, dev, bank=True)
    probe = _knn(q, r, k, dev, "probe")
    direct = _knn(q, r, k, dev, "direct")
    for name, got in (("auto", auto), ("probe", probe), ("direct", direct)):
        assert np.array_equal(got[1], want[1]), f"{name}: ids differ from the contract"
        assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{name}: distance bits differ from the contract"
        assert sum(got[2]) == nq
    assert direct[2] == (0, 0, nq)
    if sure:      # a condition, not a report: a fast path that never certifies cannot hide behind the direct path
        assert auto[2] == (nq, 0, 0) and probe[2] == (nq, 0, 0), (auto[2], probe[2])
    if nr <= C.probe_size(k, nr):
        assert auto[2] == (0, 0, nq) and probe[2] == (nq, 0, 0)       # too small for a sweep; forced, the probe holds the whole bank


def test_far_cluster_is_not_certified_and_still_exact(dev):
    _lib, ops = _ops()
    q, r = C.far_cluster()
    want = C.knn(q, r, 5)
    for path in (None, "probe"):
        D, I, rows = _knn(q, r, 5, dev, path)
        assert _same((D, I), want) and rows == (0, 0, len(q)), (path, rows)
    radius = float(np.median(want[0][:, 4]))
    lims, Dr, Ir = C.range_search(q, r, radius)
    assert 0 < lims[-1] < q.shape[0] * r.shape[0]
    for path in (None, "probe", "direct"):
        with _lib.option("VSC_L2_PATH", path):
            gl, gd, gi = ops.range_search_l2(_t(q, dev), _t(r, dev), radius)
            assert np.array_equal(gl.cpu().numpy(), lims) and np.array_equal(gi.cpu().numpy(), Ir) and np.array_equal(_bits(gd), _bits(Dr)), path
            assert ops.range_count_l2(_t(q, dev), _t(r, dev), radius) == lims[-1]


def test_wider_probe_certifies_what_the_first_cannot(dev):
    _lib, ops = _ops()
    q, r = C.middle_cluster()
    want = C.knn(q, r, 5)
    first_hi, first_lo, wide_sure = C.path_bounds(q, r, 5)           # (0, 0, >= 8): tests/test_l2_search_cpu.py
    D, I, rows = _knn(q, r, 5, dev, bank=True)
    assert _same((D, I), want) and sum(rows) == len(q)
    assert first_lo <= rows[0] <= first_hi and rows[1] >= wide_sure > 0, rows
    with _lib.option("VSC_L2_WIDE", "0"):                            # without it the same rows take the direct path: the same bytes
        D, I, rows0 = _knn(q, r, 5, dev)
    assert _same((D, I), want) and rows0 == (rows[0], 0, rows[1] + rows[2])


def test_edges(dev):
    _lib, ops = _ops()
    rng = np.random.RandomState(9)
    r = (rng.randn(40, 6) * 2).astype(np.float32)
    r[30] = r[3]                                                      # duplicate rows: the lower id first
    r[20] = 0.0
    q = np.stack([r[3], r[11], np.zeros(6, np.float32), rng.randn(6).astype(np.float32)])
    for path in (None, "probe", "direct"):
        D, I, _ = _knn(q, r, 4, dev, path)
        assert _same((D, I), C.knn(q, r, 4)), path
        assert I[0, :2].tolist() == [3, 30] and D[0, 0] == 0.0 and D[0, 1] == 0.0 and I[1, 0] == 11 and D[1, 0] == 0.0
        assert I[2, 0] == 20 and D[2, 0] == 0.0
        # k > nr: padding
        D, I, _ = _knn(q, r[:5], 9, dev, path)
        assert _same((D, I), C.knn(q, r[:5], 9)) and (I[:, 5:] == -1).all() and (D[:, 5:] == FLT_MAX).all()
        # ref_id_offset
        D, I, _ = _knn(q, r, 4, dev, path, offset=1 << 33)
        assert _same((D, I), C.knn(q, r, 4, ref_id_offset=1 << 33))
        # a NaN row and an overflowing row are never reported; a row of huge but finite norm is, where its distance is finite
        bad = r.copy()
        bad[3, 2] = np.nan
        bad[11] = 3e38
        bad[12] = 1.5e19
        qq = np.concatenate([q, np.full((1, 6), 1.5e19, np.float32), np.full((1, 6), np.nan, np.float32)])
        D, I, _ = _knn(qq, bad, 40, dev, path)
        want = C.knn(qq, bad, 40)
        assert _same((D, I), want) and not np.isin(I, (3, 11)).any() and I[4, 0] == 12 and D[4, 0] == 0.0 and (I[5] == -1).all()
        assert np.isfinite(D).all()
    # nq = 0 and nr = 0
    D, I = ops.knn_l2(torch.empty((0, 6), device=dev), _t(r, dev), 3)
    assert D.shape == (0, 3) and I.shape == (0, 3)
    D, I = ops.knn_l2(_t(q, dev), torch.empty((0, 6), device=dev), 3)
    assert (D.cpu().numpy() == FLT_MAX).all() and (I.cpu().numpy() == -1).all()
    for a, b in ((torch.empty((0, 6), device=dev), _t(r, dev)), (_t(q, dev), torch.empty((0, 6), device=dev))):
        lims, Dr, Ir = ops.range_search_l2(a, b, 5.0)
        assert lims.cpu().tolist() == [0] * (a.shape[0] + 1) and Dr.numel() == 0 and Ir.numel() == 0


def test_range(dev):
    _lib, ops = _ops()
    q, r = C.flat_l2_data()
    qd, rd = _t(q, dev), _t(r, dev)
    full = C.dist_matrix(q, r)
    aug, _, mx = ops.l2_augment(rd)
    for path in (None, "direct"):
        with _lib.option("VSC_L2_PATH", path):
            for radius, bank in ((120.0, (aug, mx)), (120.0, None), (float(full.max()) * 2, None), (np.inf, None)):   # .. every pair a hit
                lims, D, I = ops.range_search_l2(qd, rd, radius, ref_id_offset=7, capacity=2, bank=bank)     # capacity too small first
                wl, wd, wi = C.range_from(full, radius, 7)
                assert np.array_equal(lims.cpu().numpy(), wl) and np.array_equal(I.cpu().numpy(), wi) and np.array_equal(_bits(D), _bits(wd))
            assert C.range_from(full, np.inf)[0][-1] == q.size // q.shape[1] * len(r)
            for radius in (0.0, -1.0, float(np.nextafter(np.float32(0), np.float32(1))), np.nan):            # no hit (but the exact match at 0)
                lims, D, I = ops.range_search_l2(qd, rd, radius)
                wl, wd, wi = C.range_from(full, radius)
                assert np.array_equal(lims.cpu().numpy(), wl) and np.array_equal(I.cpu().numpy(), wi)
            # the radius equal to one pair's distance bits excludes that pair, the next float includes it
            edge = np.float32(full[2, 40])
            for radius, inside in ((edge, False), (np.nextafter(edge, np.float32(np.inf)), True)):
                lims, D, I = ops.range_search_l2(qd, rd, float(radius))
                mine = I[lims[2]:lims[3]].cpu().numpy()
                assert (40 in mine) == inside and np.array_equal(I.cpu().numpy(), C.range_from(full, radius)[2])
            # capacity 0 counts only; a capacity that is too small writes nothing
            lib = _lib.load()
            total = ctypes.c_int64(-1)
            lims = torch.full((len(q) + 1,), -5, dtype=torch.int64, device=dev)
            D = torch.full((2,), -3.0, device=dev)
            I = torch.full((2,), -3, dtype=torch.int64, device=dev)
            want_total = int((full < np.float32(120.0)).sum())
            _lib.check(lib.vsc_range_search_l2_f32(None, _lib.ptr(qd), len(q), _lib.ptr(rd), len(r), 24, 120.0, 0, None, None, _lib.ptr(lims), None, None,
                                                   0, ctypes.byref(total)))
            assert total.value == want_total > 2
            _lib.check(lib.vsc_range_search_l2_f32(None, _lib.ptr(qd), len(q), _lib.ptr(rd), len(r), 24, 120.0, 0, None, None, _lib.ptr(lims), _lib.ptr(D),
                                                   _lib.ptr(I), 2, ctypes.byref(total)))
            torch.cuda.synchronize()
            assert total.value == want_total and (D == -3.0).all() and (I == -3).all()


def _guarded(values, dev, odd):
    """`values` inside a larger allocation between guard bands, its first element `odd` elements past an aligned address"""
    import test_gpu_abi_placement as P
    t = torch.from_numpy(np.ascontiguousarray(values))
    nbytes, es = t.numel() * t.element_size(), t.element_size()
    raw = torch.empty(nbytes + 2 * P.GUARD + P.ALIGN + odd * es, dtype=torch.uint8, device=dev)
    off = P.GUARD + (-(raw.data_ptr() + P.GUARD)) % P.ALIGN + odd * es
    raw.fill_(P.PATTERN)
    view = raw[off:off + nbytes].view(t.dtype).reshape(t.shape)
    view.copy_(t)
    intact = lambda: bool((raw[:off] == P.PATTERN).all()) and bool((raw[off + nbytes:] == P.PATTERN).all())
    return view, intact


def test_placement_guards_stream_interleaving_and_repeats(dev):
    _lib, ops = _ops()
    lib = _lib.load()
    nq, nr, d, k = 17, 500, 24, 9
    q, r, want, _ = _case(nq, nr, d, k)
    full = C.dist_matrix(q, r)
    wl, wd, wi = C.range_from(full, 120.0)
    # operands and outputs at odd element offsets between guard bands
    qv, q_ok = _guarded(q, dev, 1)
    rv, r_ok = _guarded(r, dev, 3)
    Dv, D_ok = _guarded(np.full((nq, k), np.nan, np.float32), dev, 1)
    Iv, I_ok = _guarded(np.full((nq, k), -9, np.int64), dev, 1)
    lv, l_ok = _guarded(np.full(nq + 1, -9, np.int64), dev, 1)
    hd, hd_ok = _guarded(np.full(len(wd), np.nan, np.float32), dev, 1)
    hi, hi_ok = _guarded(np.full(len(wd), -9, np.int64), dev, 3)
    total = ctypes.c_int64(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    for path in (None, "probe", "direct"):
        with _lib.option("VSC_L2_PATH", path):
            Dv.fill_(float("nan"))
            _lib.check(lib.vsc_knn_l2_f32(None, P(qv), nq, P(rv), nr, d, k, 0, None, None, P(Dv), P(Iv)))
            _lib.check(lib.vsc_range_search_l2_f32(None, P(qv), nq, P(rv), nr, d, 120.0, 0, None, None, P(lv), P(hd), P(hi), len(wd), ctypes.byref(total)))
            torch.cuda.synchronize()
            assert _same((Dv, Iv.cpu().numpy()), want) and total.value == len(wd)
            assert np.array_equal(lv.cpu().numpy(), wl) and np.array_equal(hi.cpu().numpy(), wi) and np.array_equal(_bits(hd), _bits(wd))
            assert all(f() for f in (q_ok, r_ok, D_ok, I_ok, l_ok, hd_ok, hi_ok)), "a guard band changed"
            assert np.array_equal(qv.cpu().numpy(), q) and np.array_equal(rv.cpu().numpy(), r)
    # a non-default stream
    qd, rd = _t(q, dev), _t(r, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        D, I = ops.knn_l2(qd, rd, k)
        lims, Dr, Ir = ops.range_search_l2(qd, rd, 120.0)
    side.synchronize()
    assert _same((D, I.cpu().numpy()), want) and np.array_equal(Ir.cpu().numpy(), wi) and np.array_equal(_bits(Dr), _bits(wd))
    # inner-product and L2 entries interleaved over the shared scratch, three runs with identical bytes
    ip_first = ops.knn_ip(qd, rd, k)
    ipr_first = ops.range_search_ip(qd, rd, 30.0)
    ip_path = lib.vsc_knn_last_path()
    for run in range(3):
        order = [("l2", "ip", "rl2", "rip"), ("rip", "rl2", "ip", "l2"), ("ip", "l2", "l2", "rip", "rl2", "ip")][run]
        if run == 2:
            lib.vsc_search_release_scratch()
        for what in order:
            if what == "l2":
                D, I = ops.knn_l2(qd, rd, k)
                assert _same((D, I.cpu().numpy()), want) and lib.vsc_knn_last_path() == ip_path
            elif what == "rl2":
                lims, Dr, Ir = ops.range_search_l2(qd, rd, 120.0)
                assert np.array_equal(lims.cpu().numpy(), wl) and np.array_equal(Ir.cpu().numpy(), wi) and np.array_equal(_bits(Dr), _bits(wd))
            elif what == "ip":
                D, I = ops.knn_ip(qd, rd, k)
                assert torch.equal(D.view(torch.int32), ip_first[0].view(torch.int32)) and torch.equal(I, ip_first[1])
            else:
                got = ops.range_search_ip(qd, rd, 30.0)
                assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                           for a, b in zip(got, ipr_first))


def test_across_workgroups_and_bank_splits(dev):
    """256 x 65 536, d = 64, k = 100: the sweep's pre-filter path, many workgroups, several bank splits."""
    nq, nr, d, k = 256, 65536, 64, 100
    q, r = C.unit(21, nq, d), C.unit(22, nr, d)
    D, I, rows = _knn(q, r, k, dev, bank=True)
    assert sum(rows) == nq
    print("rows by path (first probe, wider probe, direct):", rows)
    sample = [0, 1, 63, 64, 127, 128, 200, 255]
    want = C.knn(q[sample], r, k)
    assert _same((D[sample], I[sample]), want)
    assert (np.diff(D.astype(np.float64), axis=1) >= 0).all() and (I >= 0).all() and (I < nr).all()
    assert all(len(set(row.tolist())) == k for row in I)
    ties = np.diff(D, axis=1) == 0
    assert (np.diff(I, axis=1)[ties] > 0).all()


def test_python_layer(dev):
    from vsc.index import METRIC_L2, FlatIPBank, VideoFeature, VideoIndex
    q, r = C.flat_l2_data()
    host, hip = FlatIPBank(24, METRIC_L2), FlatIPBank(24, METRIC_L2, l2="hip")
    for bank in (host, hip):
        bank.add(r[:200])
        bank.add(r[200:])

    def ulps(a, b):
        return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))

    Dh, Ih = host.search(q, 9)
    D, I = hip.search(q, 9)
    assert np.array_equal(I, Ih) and ulps(D, Dh).max() <= 4 and _same((D, I), C.knn(q, r, 9))
    rows_h, ids_h, dist_h = host.range_search(q, 120.0)
    rows, ids, dist = hip.range_search(q, 120.0)
    assert np.array_equal(rows, rows_h) and np.array_equal(ids, ids_h) and ulps(dist, dist_h).max() <= 4
    assert hip.range_count(q, 120.0) == len(rows) == host.range_count(q, 120.0)
    Dd, Id = hip.search_device(q, 9)
    assert Dd.is_cuda and np.array_equal(Id.cpu().numpy(), I) and np.array_equal(_bits(Dd), _bits(D))
    rd, idd, dd = hip.range_search_device(q, 120.0)
    assert rd.is_cuda and np.array_equal(rd.cpu().numpy(), rows) and np.array_equal(idd.cpu().numpy(), ids) and np.array_equal(_bits(dd), _bits(dist))
    adopted = FlatIPBank(24, METRIC_L2, l2="hip")
    adopted.add(r)
    adopted.adopt_device_rows(_t(r, dev))
    assert adopted.adopted
    Da, Ia = adopted.search(q, 9)
    assert np.array_equal(Ia, I) and np.array_equal(_bits(Da), _bits(D))
    with pytest.raises(ValueError):
        adopted.adopt_device_rows(_t(r[:10], dev))

    feats = np.array([[[1, 2, 3], [4, 5, 6], [7, 8, 9]], [[11, 12, 13], [14, 15, 16], [17, 18, 19]],
                      [[111, 112, 113], [114, 115, 116], [117, 118, 119]]], np.float32)   # the reference's tests/test_index.py data
    mk = lambda pre: [VideoFeature(video_id=f"{pre}{i:06d}", feature=f, timestamps=np.arange(3, dtype=np.float32)) for i, f in enumerate(feats)]
    for gk in (1, -1, 4):
        res = {}
        for form in ("host", "hip"):
            idx = VideoIndex(3, "Flat", METRIC_L2, l2=form)
            idx.add(mk("R"))
            res[form] = idx.search(mk("Q"), gk)
            assert res[form] and all(x.query_id[1:] == x.ref_id[1:] for x in res[form])
        assert res["hip"] == res["host"]
    hits = idx._global_threshold_knn_search(feats.reshape(9, 3), 9)
    assert sorted((i, j) for i, j, _ in hits) == [(i, i) for i in range(9)] and all(s == 0.0 for _, _, s in hits)
