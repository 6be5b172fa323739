"""The view decisions on the device (csrc/view_decide.hip, ops.view_decide, ``detect_views(decisions="hip")``,
``extract_query_feats.py --view_decisions hip``): the entry through ctypes against the executable contract
(tests/view_decide_contract.py) on every case of tests/view_decide_cases.py -- the 720 x 1280 letterbox and the maps around the
8192-element boundary included -- between 0xFF guard bands: boxes, counts, status and the bits of the trace; one batched call
against the single calls; two runs against each other; detect_views with maps and decisions from the device against the default
path and the fixture; the entry point's files byte for byte."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import view_cases  # noqa: E402
import view_decide_cases as cases  # noqa: E402
import view_decide_contract as C  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 512                     # bytes of 0xFF on both sides of every output
P = ctypes.c_void_p
FIXTURE = os.path.join(HERE, "golden", "view_preprocess.json")


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def guarded(nbytes, dev):
    whole = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + nbytes]


def run_entry(var_dev, count_dev, items, max_views, dev, trace=True):
    """one vsc_view_decide_f64 call with guarded outputs on the null stream -> (rc, boxes [n, max_views, 4], counts, status, trace
    [n, 8] (all 0xFF bytes with trace=False), guards intact)"""
    from vsc_hip import _lib
    lib = _lib.load()
    items = np.ascontiguousarray(items, np.int64).reshape(-1, 6)
    n = len(items)
    out = {k: guarded(b, dev) for k, b in (("boxes", 16 * n * max(max_views, 1)), ("counts", 4 * n), ("status", 4 * n), ("trace", 64 * n))}
    p = {k: P(body.data_ptr()) for k, (_, body) in out.items()}
    if not trace:
        p["trace"] = None
    h = P()
    _lib.check(lib.vsc_view_decide_create(None, ctypes.byref(h)))
    try:
        rc = lib.vsc_view_decide_f64(h, P(var_dev.data_ptr()), var_dev.numel(), P(count_dev.data_ptr()), count_dev.numel(), items.ctypes.data,
                                     n, max_views, p["boxes"], p["counts"], p["status"], p["trace"])
    finally:
        lib.vsc_view_decide_destroy(h)              # host state only: what is enqueued does not refer to it
    torch.cuda.synchronize()
    intact = True
    for whole, _ in out.values():
        w = whole.cpu().numpy()
        intact = intact and bool((w[:GUARD] == 0xFF).all() and (w[len(w) - GUARD:] == 0xFF).all())
    host = {k: body.cpu().numpy() for k, (_, body) in out.items()}
    return (rc, host["boxes"].view(np.int32).reshape(n, max(max_views, 1), 4), host["counts"].view(np.int32), host["status"].view(np.int32),
            host["trace"].view(np.float64).reshape(n, 8), intact)


def assert_item(name, boxes, count, status, trace, want=None):
    want_boxes, want_status, want_trace = cases.expected(want or name)
    print(f"{name}: views {count} status {status} contract {len(want_boxes)} / {want_status}")
    assert status == want_status, (name, status)
    assert count == len(want_boxes), (name, count, want_boxes)
    assert boxes[:count].tolist() == [list(b) for b in want_boxes], (name, boxes[:count].tolist(), want_boxes)
    assert (boxes[count:] == -1).all(), (name, "the tail is not -1")
    if trace is not None:
        assert np.array_equal(C.bits(trace), C.bits(want_trace)), (name, "trace bits", trace, want_trace)


def upload(case, dev):
    return torch.from_numpy(np.array(case["var"]).reshape(-1)).to(dev), torch.from_numpy(np.array(case["count"]).reshape(-1)).to(dev)


@pytest.mark.parametrize("name", cases.names())
def test_entry_equals_the_contract_between_guard_bands(dev, name):
    """boxes, counts, status and trace bits; with a NULL trace the same boxes and nothing written elsewhere; two runs, the same bytes"""
    case = cases.get(name)
    h, w = case["var"].shape
    var, count = upload(case, dev)
    item = [(0, 0, h, w, case["m"], case["n"])]
    rc, boxes, counts, status, trace, intact = run_entry(var, count, item, case["max_views"], dev)
    assert rc == 0 and intact, (name, rc, "a guard band changed" if rc == 0 else "refused")
    assert_item(name, boxes[0], int(counts[0]), int(status[0]), trace[0])
    rc, boxes2, counts2, status2, trace2, intact = run_entry(var, count, item, case["max_views"], dev, trace=False)
    assert rc == 0 and intact and np.array_equal(boxes2, boxes) and np.array_equal(counts2, counts) and np.array_equal(status2, status)
    assert (trace2.view(np.uint8) == 0xFF).all(), "a NULL output was written somewhere else"
    rc, boxes3, counts3, status3, trace3, intact = run_entry(var, count, item, case["max_views"], dev)
    assert rc == 0 and intact and np.array_equal(boxes3, boxes) and np.array_equal(counts3, counts) and np.array_equal(status3, status)
    assert np.array_equal(C.bits(trace3), C.bits(trace)), (name, "two runs, different bytes")


def test_one_batched_call_equals_the_single_calls(dev):
    """every case in one call at odd element offsets -- more items than one launch holds, the 720p map among small ones; the
    engineered case has room at max_views = 64 and equals its twin"""
    sel = cases.names() + ["width_7", "frames_4", "height_9", "random_3"] * 3
    assert len(sel) > 64
    var, count, items = cases.batch(sel)
    assert any(int(v) % 2 for v in items[:, 0]) and any(int(v) % 2 for v in items[:, 1])
    rc, boxes, counts, status, trace, intact = run_entry(torch.from_numpy(var).to(dev), torch.from_numpy(count).to(dev), items, C.MAX_VIEWS, dev)
    assert rc == 0 and intact
    for k, name in enumerate(sel):
        assert_item(name, boxes[k], int(counts[k]), int(status[k]), trace[k], want="stack3" if name in cases.ENGINEERED else None)


def test_refusals_write_nothing(dev):
    case = cases.get("width_9")
    h, w = case["var"].shape
    var, count = upload(case, dev)
    good = (0, 0, h, w, 20, 8)
    bad = [([(0, 0, 4097, 1, 20, 8)], 64), ([(0, 0, h, 0, 20, 8)], 64), ([(0, 0, h, w, 0, 8)], 64), ([(0, 0, h, w, 256, 8)], 64),
           ([(1, 0, h, w, 20, 8)], 64), ([(0, 1, h, w, 20, 8)], 64), ([(-1, 0, 1, 1, 20, 8)], 64), ([good], 0), ([good], 65),
           ([good, (0, 0, h, 4097, 20, 8)], 64)]
    for items, max_views in bad:
        rc, boxes, counts, status, trace, intact = run_entry(var, count, items, max_views, dev)
        assert rc != 0 and intact, (items, max_views)
        assert all((a.view(np.uint8) == 0xFF).all() for a in (boxes, counts, status, trace)), ("a refused call wrote", items)
    from vsc_hip import _lib, ops
    with pytest.raises(_lib.VscHipError, match="view_decide"):
        ops.view_decide(var, count, [(0, 0, h + 1, w, 20, 8)])
    b, c, s, t = ops.view_decide(var, count, [good], trace=True)
    assert_item("width_9", b[0].cpu().numpy(), int(c[0]), int(s[0]), t[0].cpu().numpy())


def test_detect_views_with_device_decisions_equals_the_host_path(dev, monkeypatch):
    """the 21 recipes' frames: maps and decisions both from the device, the boxes equal the default path's and the fixture's; the
    device path downloads no map; a video the kernel leaves to the host (status 1) gets the host path's boxes"""
    from src import image_preprocess as ip
    from vsc_hip import ops
    with open(FIXTURE) as f:
        fixture = json.load(f)["cases"]
    assert len(fixture) == 21
    frames = {c["name"]: torch.from_numpy(view_cases.frames(c)).to(dev) for c in fixture}
    host = {name: ip.detect_views(d) for name, d in frames.items()}
    c0 = fixture[0]
    var, count = ops.view_maps(frames[c0["name"]], ip.canny_frames(c0["n"]))
    var_d, count_d = ops.view_maps_dev(frames[c0["name"]], ip.canny_frames(c0["n"]))
    assert np.array_equal(C.bits(var_d.cpu().numpy()), C.bits(var)) and np.array_equal(count_d.cpu().numpy(), count)
    calls = []
    real = ops.view_decide
    monkeypatch.setattr(ops, "view_decide", lambda *a, **k: calls.append(1) or real(*a, **k))
    with monkeypatch.context() as m:
        m.setattr(ops, "view_maps", lambda *a, **k: pytest.fail("the device decisions downloaded the maps"))
        for c in fixture:
            changed, boxes = ip.detect_views(frames[c["name"]], decisions="hip")
            assert (changed, boxes) == host[c["name"]], c["name"]
            assert (changed, [list(b) for b in boxes]) == (c["changed"], c["boxes"]), c["name"]
    assert len(calls) == sum(1 for c in fixture if c["n"] >= 5)
    monkeypatch.setattr(ops, "VIEW_DECIDE_MAX_VIEWS", 2)
    assert ip.detect_views(frames["stack3_vertical"], decisions="hip") == host["stack3_vertical"] and len(host["stack3_vertical"][1]) == 3
    views = ip.HipViews(dev, decisions="hip")
    boxes, out = views(torch.from_numpy(view_cases.frames(fixture[3])), [32])
    assert [list(b) for b in boxes] == fixture[3]["boxes"] and out[32].shape[0] == len(boxes) * fixture[3]["n"]


def test_extract_query_feats_writes_the_same_files_with_device_decisions(tmp_path):
    """--preprocess hip --view_decisions hip against --preprocess hip alone on the small zips of
    test_extract_query_feats_with_hip_views: every array of every .npz byte for byte (the zip container around them carries
    the clock's time stamps, so the members are compared, not the container)"""
    import extract_query_feats as E
    from test_gpu_uap_e2e import GOLD, _checkpoints, _pca_pickle
    from test_gpu_view_preprocess import _cases, _write_zips
    g = np.load(GOLD)
    root = str(tmp_path)
    recipes = {c["name"]: c for c in _cases()}
    names = {"Q300001": "letterbox", "Q300002": "stack2_vertical", "Q300003": "plain"}
    zips = os.path.join(root, "zips")
    _write_zips(zips, {vid: view_cases.frames(recipes[name]) for vid, name in names.items()})
    ids = os.path.join(root, "ids.txt")
    with open(ids, "w") as f:
        f.write("\n".join(names) + "\n")
    models = _checkpoints(g, root)
    pca_path = os.path.join(root, "pca_model.pkl")
    _pca_pickle(g, pca_path)
    spec = [f"{arch}:{fmt}:{ckpt}" for _, arch, fmt, ckpt in models]
    outs = {}
    for mode in ("host", "hip"):
        outs[mode] = os.path.join(root, "out_" + mode)
        E.main(E.build_parser().parse_args(["--split", "test", "--models"] + spec + ["--pca_model", pca_path, "--zip_prefix", zips, "--input_file", ids,
                                            "--output_dir", outs[mode], "--workers", "0", "--preprocess", "hip", "--view_decisions", mode]))
    files = sorted(os.path.relpath(os.path.join(d, f), outs["host"]) for d, _, fs in os.walk(outs["host"]) for f in fs if f.endswith(".npz"))
    assert len(files) >= len(models) + 1, files
    for rel in files:
        with np.load(os.path.join(outs["host"], rel), allow_pickle=False) as a, np.load(os.path.join(outs["hip"], rel), allow_pickle=False) as b:
            assert sorted(a.files) == sorted(b.files) and a.files, rel
            for key in a.files:
                assert (a[key].dtype, a[key].shape) == (b[key].dtype, b[key].shape) and a[key].tobytes() == b[key].tobytes(), (rel, key)
