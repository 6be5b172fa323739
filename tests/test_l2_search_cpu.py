"""The exact L2 search without a GPU: the contract (tests/l2_search_contract.py) against a float64 brute force, the bound `slack` held
to its claim, the certificate rule on the reference arithmetic alone -- the facts that let tests/test_gpu_l2_search.py demand that
the fast path ran -- and the l2= plumbing and the entries' refusals."""
import ctypes

import numpy as np
import pytest

import l2_search_contract as C


def _d64(q, r):
    return ((q[:, None, :].astype(np.float64) - r[None].astype(np.float64)) ** 2).sum(-1)


@pytest.mark.parametrize("nq,nr,d,k", [(17, 500, 24, 9), (5, 300, 33, 40), (8, 400, 512, 10)])
def test_contract_against_float64_brute_force(nq, nr, d, k):
    """Distances within d 2^-24 relative of float64 (the chain rounds each difference once and each of its d steps once; at d >= 24 the
    accumulated error of random data stays far inside d half-ulps -- the worst case is (d + 2) 2^-24, which d = 1 could reach, so the
    cases start at 24).  Ids equal float64's wherever float64 separates the neighbours by more than the chain's rounding: rows whose
    k + 1 smallest float64 distances are pairwise further apart than 2 (d + 2) 2^-24 of the larger one."""
    rng = np.random.RandomState(d)
    q, r = (rng.randn(nq, d) * 3).astype(np.float32), (rng.randn(nr, d) * 3).astype(np.float32)
    q[0] = r[7]
    D, I = C.knn(q, r, k)
    d64 = _d64(q, r)
    order = np.argsort(d64, axis=1, kind="stable")[:, :k + 1]
    near = np.take_along_axis(d64, order, 1)
    separated = (np.diff(near, axis=1) > 2 * (d + 2) * 2.0 ** -24 * near[:, 1:]).all(1)
    assert separated.sum() >= nq - 2, "the case checks (almost) nothing"
    assert np.array_equal(I[separated], order[separated, :k])
    assert I[0, 0] == 7 and D[0, 0] == 0.0
    full = C.dist_matrix(q, r)
    assert (np.abs(full.astype(np.float64) - d64) <= d * 2.0 ** -24 * d64).all()
    assert (np.diff(D.astype(np.float64), axis=1) >= 0).all()
    # a slice of a larger call is the same bits; range is the strict cut of the same distances
    assert np.array_equal(C.dist_matrix(q[2:5], r[10:60]).view(np.uint32), full[2:5, 10:60].view(np.uint32))
    radius = float(np.median(D[:, -1]))
    lims, Dr, Ir = C.range_search(q, r, radius)
    assert lims[-1] == (full < np.float32(radius)).sum() and (Dr < np.float32(radius)).all()
    for i in range(nq):
        assert np.array_equal(Ir[lims[i]:lims[i + 1]], np.flatnonzero(full[i] < np.float32(radius)))


def test_contract_order_padding_and_non_finite_distances():
    r = np.array([[1, 0], [0, 1], [1, 0], [np.nan, 0], [3e38, -3e38], [2, 0]], np.float32)
    q = np.array([[1, 0], [0, 0]], np.float32)
    D, I = C.knn(q, r, 8, ref_id_offset=100)
    assert I[0].tolist() == [100, 102, 105, 101, -1, -1, -1, -1] and D[0, :4].tolist() == [0.0, 0.0, 1.0, 2.0]
    assert I[1].tolist() == [100, 101, 102, 105, -1, -1, -1, -1]              # equal distances: the lower id first
    assert (D[:, 4:] == C.FLT_MAX).all()
    lims, Dr, Ir = C.range_search(q, r, np.inf)
    assert lims.tolist() == [0, 4, 8] and Ir[:4].tolist() == [0, 1, 2, 5]     # inf < inf is false; NaN never compares


def _adversarial(d):
    rng = np.random.RandomState(100 + d)
    sets = []
    q, r = C.far_cluster(seed=d, nr=200, nq=8, d=d)
    sets.append((q, r))
    scale = 10.0 ** rng.uniform(-3, 3, size=(200, 1))                         # mixed norms 1e-3 .. 1e3
    r = (rng.randn(200, d) * scale).astype(np.float32)
    q = (rng.randn(8, d) * 10.0 ** rng.uniform(-3, 3, size=(8, 1))).astype(np.float32)
    sets.append((q, r))
    sets.append((np.concatenate([q, r[:4]]), np.concatenate([r, -r[:50], r[:50] * np.float32(1 + 2.0 ** -20)])))   # cancellation: r against ~r, -r
    return sets


@pytest.mark.parametrize("d", [1, 24, 512])
def test_slack_bounds_the_expanded_form(d):
    """|expanded score + chain distance| <= slack on far clusters, mixed norms and near-cancelling pairs."""
    worst = 0.0
    for q, r in _adversarial(d):
        e, dist = C.expanded_matrix(q, r).astype(np.float64), C.dist_matrix(q, r).astype(np.float64)
        qn, rmax = C.norms(q), C.norms(r).max()
        s = np.array([C.slack(d, v, rmax) for v in qn])[:, None]
        assert np.isfinite(s).all() and (s > 0).all()
        ratio = (np.abs(e + dist) / s).max()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (d, ratio)
    print(f"d={d}: worst |expanded + dist| / slack = {worst:.3g}")


def test_slack_is_infinite_where_there_is_no_bound():
    assert C.slack(8, np.inf, 1.0) == np.inf and C.slack(8, 1.0, np.nan) == np.inf and C.slack(8, 1e38, 1e38) == np.inf
    assert np.isfinite(C.slack(4094, 1.0, 1.0)) and C.slack(16, 0.0, 0.0) > 0


def test_certificate_rule_on_the_reference_arithmetic():
    """Every row is certified at kk = max(k + 8, 2k) on the inputs the GPU tests call certifiable; none on the far cluster."""
    q, r = C.flat_l2_data()
    assert C.certified(q, r, 9).all()
    q, r = C.unit(11, 16, 512), C.unit(12, 3000, 512)
    assert C.certified(q, r, 10).all() and C.certified(q, r, 100).all()
    assert C.certified(C.unit(13, 16, 33), C.unit(14, 5000, 33), 10).all()
    q, r = C.far_cluster()
    assert not C.certified(q, r, 5).any()
    # ... and there the heuristic probe of the host form does lose true neighbours: the reason the rule exists
    e = C.expanded_matrix(q, r)
    _, want = C.knn(q, r, 5)
    kk = C.probe_size(5, len(r))
    lost = sum(len(set(want[i]) - set(np.lexsort((np.arange(len(r)), -e[i].astype(np.float64)))[:kk])) for i in range(len(q)))
    assert lost > 0
    assert C.certified(q, r[:10], 5).all()                                    # a probe that holds the whole bank
    assert C.wide_probe_size(5, 300) == 256 and C.wide_probe_size(5, 256) == 0 and C.wide_probe_size(100, 3000) == 800
    assert C.wide_probe_size(1024, 5000) == 0 and C.path_bounds(q, r, 5) == (0, 0, 0)
    # ... and a cluster in between, which only the wider probe certifies -- with a factor 2 of margin on slack either way
    q, r = C.middle_cluster()
    first_hi, first_lo, wide_sure = C.path_bounds(q, r, 5)
    assert first_hi == 0 and first_lo == 0 and wide_sure >= 8


def test_l2_argument_plumbing():
    from vsc.index import L2_FORMS, METRIC_INNER_PRODUCT, METRIC_L2, FlatIPBank, VideoIndex
    assert L2_FORMS == ("host", "hip")
    for bad in ("gpu", "", None, "HIP"):
        with pytest.raises(ValueError, match="l2"):
            FlatIPBank(8, METRIC_L2, l2=bad)
        with pytest.raises(ValueError, match="l2"):
            VideoIndex(8, "Flat", METRIC_L2, l2=bad)
    assert FlatIPBank(8, METRIC_L2).l2 == "host" and not FlatIPBank(8, METRIC_L2).l2_native
    assert FlatIPBank(8, METRIC_L2, l2="hip").l2_native and not FlatIPBank(8, METRIC_INNER_PRODUCT, l2="hip").l2_native
    assert VideoIndex(8, "Flat", METRIC_L2, l2="hip").index.l2_native and not VideoIndex(8, "Flat", METRIC_L2).index.l2_native
    host = FlatIPBank(8, METRIC_L2)
    host.add(np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError, match="l2='hip'"):
        host.search_device(np.zeros((1, 8), np.float32), 1)
    with pytest.raises(ValueError, match="l2='hip'"):
        host.range_search_device(np.zeros((1, 8), np.float32), 1.0)
    with pytest.raises(ValueError, match="l2='hip'"):
        host.adopt_device_rows(None)
    with pytest.raises(ValueError, match="selection='hip'"):                  # out of scope here: stays refused
        VideoIndex(8, "Flat", METRIC_L2, selection="hip", l2="hip")
    bank = FlatIPBank(8, METRIC_L2, l2="hip")
    bank.add(np.ones((2, 8), np.float32))
    bank._l2_aug = object()
    bank.add(np.ones((2, 8), np.float32))
    assert bank._l2_aug is None and bank.ntotal == 4                          # add() drops the device bank's augmentation
    from vsc_hip import ops
    assert all(callable(getattr(ops, n)) for n in ("l2_augment", "knn_l2", "range_search_l2", "range_count_l2", "knn_l2_last_path"))


def test_entries_refuse_by_name_before_touching_the_device():
    """Limits of the header: k <= 1024, d <= 4096 (4094 with augmented rows or on the forced probe path), operands that come
    together.  The refusals come before any device call, so they run here; the pointers are never read."""
    from vsc_hip import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    total = ctypes.c_int64(-7)

    def refused(rc, text):
        assert rc != 0 and text in lib.vsc_last_error().decode(), (rc, lib.vsc_last_error())

    refused(lib.vsc_knn_l2_f32(None, fake, 4, fake, 9, 8, 1025, 0, None, None, fake, fake), "k=1025 out of range")
    refused(lib.vsc_knn_l2_f32(None, fake, 4, fake, 9, 8, 0, 0, None, None, fake, fake), "k=0 out of range")
    refused(lib.vsc_knn_l2_f32(None, fake, 4, fake, 9, 4097, 5, 0, None, None, fake, fake), "dimension 4097 unsupported")
    refused(lib.vsc_knn_l2_f32(None, fake, 4, fake, 9, 0, 5, 0, None, None, fake, fake), "dimension 0 unsupported")
    refused(lib.vsc_knn_l2_f32(None, fake, 4, fake, 9, 4095, 5, 0, fake, fake, fake, fake), "up to d = 4094")
    refused(lib.vsc_knn_l2_f32(None, fake, 4, fake, 9, 8, 5, 0, fake, None, fake, fake), "come together")
    refused(lib.vsc_knn_l2_f32(None, fake, -1, fake, 9, 8, 5, 0, None, None, fake, fake), "negative row count")
    refused(lib.vsc_knn_l2_f32(None, fake, 4, fake, 9, 6, 5, 0, ctypes.c_void_p(4100), fake, fake, fake), "16-byte aligned")
    with _lib.option("VSC_L2_PATH", "probe"):
        refused(lib.vsc_knn_l2_f32(None, fake, 4, fake, 9, 4095, 5, 0, None, None, fake, fake), "VSC_L2_PATH=probe needs d <= 4094")
        refused(lib.vsc_range_search_l2_f32(None, fake, 4, fake, 9, 4096, 1.0, 0, None, None, fake, None, None, 0, ctypes.byref(total)),
                "VSC_L2_PATH=probe needs d <= 4094")
    assert _lib.get_option("VSC_L2_PATH") is None
    refused(lib.vsc_range_search_l2_f32(None, fake, 4, fake, 9, 4097, 1.0, 0, None, None, fake, None, None, 0, ctypes.byref(total)),
            "dimension 4097 unsupported")
    refused(lib.vsc_range_search_l2_f32(None, fake, 4, fake, 9, 8, 1.0, 0, None, None, fake, None, None, 5, ctypes.byref(total)),
            "capacity 5 without output buffers")
    refused(lib.vsc_range_search_l2_f32(None, fake, 4, fake, 9, 8, 1.0, 0, None, None, None, None, None, 0, ctypes.byref(total)), "null pointer")
    assert total.value == -7                                                  # nothing written
    refused(lib.vsc_l2_augment_f32(None, fake, 4, 4095, 0, fake, None, None), "dimension 4095 unsupported")
    refused(lib.vsc_l2_augment_f32(None, fake, 4, 8, 0, None, None, None), "no output")
    refused(lib.vsc_knn_l2_last_path(None), "null pointer")
    assert lib.vsc_knn_l2_f32(None, None, 0, fake, 9, 8, 5, 0, None, None, None, None) == 0      # nq == 0: nothing to do, nothing written
