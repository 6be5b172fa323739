"""Fixture of the query view preprocessing (border removal and split views), pinned on the reference (build container only):

    VSC_RUN_REFERENCE_CODE=1 python tests/golden/gen_view_golden.py [--check]

The reference's ``remove_edges``, ``split_imgs``, ``clean_imgs`` and ``image_process`` (infer/src/image_preprocess.py) are read
from /root/reference at run time: the file is pinned by SHA-256, parsed, and only those four function definitions are executed,
in a namespace that holds numpy, a ``cv2`` stand-in and a ``PIL.Image`` stand-in -- nothing of the file's header runs and no
reference text is written anywhere.

The one restated piece is Canny: the stand-in's ``cv2.Canny`` is tests/canny_cpu.py (cv2 is not installed here), the same
contract the kernel vsc_canny_count_u8 implements.  Everything above Canny -- the variance map, the frame sampling, every
decision -- is the reference's own code.  The ``Image.fromarray`` stand-in returns the array view itself, so the box of each
view is read from its data offset in the frame it was cut from.

The videos come from tests/view_cases.py; the fixture (tests/golden/view_preprocess.json) stores their recipes, frame digests,
the reference's status and boxes and the digests of both maps, no frames.  ``--check`` regenerates in memory and compares with
the committed file instead of writing it.
"""
import ast
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "vsc22-submission_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import canny_cpu  # noqa: E402
import view_cases  # noqa: E402

REFERENCE = "/root/reference"
PREP_SRC = "VSC22-Descriptor-Track-1st/infer/src/image_preprocess.py"
PREP_SHA256 = "b516f8045a16bc4850b68d7d82aec0d0d71b36e169e2daf046280dff76807ebb"
OPT_IN = "VSC_RUN_REFERENCE_CODE"
OUT = os.path.join(HERE, "view_preprocess.json")
FUNCS = ("remove_edges", "split_imgs", "clean_imgs", "image_process")


class _Cv2:
    """cv2 as the reference code sees it: Canny only, restated by tests/canny_cpu.py"""

    @staticmethod
    def Canny(img, low, high):
        return canny_cpu.canny(np.asarray(img), low, high)


class _Image:
    """PIL.Image as the reference code sees it: fromarray hands back the array view (its offset gives the box)"""

    @staticmethod
    def fromarray(a):
        return a


def load_image_process():
    """-> image_process executed from the pinned image_preprocess.py"""
    if os.environ.get(OPT_IN) != "1":
        raise RuntimeError(f"executing reference code is opt-in: set {OPT_IN}=1")
    path = os.path.join(REFERENCE, PREP_SRC)
    with open(path, "rb") as f:
        raw = f.read()
    if hashlib.sha256(raw).hexdigest() != PREP_SHA256:
        raise RuntimeError(f"{PREP_SRC} does not match its pinned SHA-256")
    tree = ast.parse(raw.decode("utf-8"), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in FUNCS]
    if sorted(d.name for d in defs) != sorted(FUNCS):
        raise RuntimeError("image_process definitions not found")
    ns = {"np": np, "cv2": _Cv2, "Image": _Image}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns["image_process"]


def _root(a):
    while a.base is not None and isinstance(a.base, np.ndarray):
        a = a.base
    return a


def box_of(view):
    """(y0, y1, x0, x1) of an [h, w, 3] view inside the [H, W, 3] frame it was sliced from"""
    root = _root(view)
    h_full, w_full = root.shape[-3], root.shape[-2]
    off = view.__array_interface__["data"][0] - root.__array_interface__["data"][0]
    row = w_full * 3
    off %= h_full * row
    y0, x0 = off // row, (off % row) // 3
    return [int(y0), int(y0 + view.shape[0]), int(x0), int(x0 + view.shape[1])]


def run_case(case, image_process):
    frames = view_cases.frames(case)
    n, h, w = frames.shape[:3]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        changed, out = image_process([f for f in frames])
    if not changed:
        return False, [[0, h, 0, w]]
    assert len(out) % n == 0
    views = [out[v * n:(v + 1) * n] for v in range(len(out) // n)]
    boxes = [box_of(v[0]) for v in views]
    for v, b in zip(views, boxes):      # every frame of a view has the same box, in frame order
        assert all(box_of(x) == b for x in v)
    return True, boxes


def maps(case):
    """(variance map digest, edge-count map digest, m) as the GPU computes them"""
    from src.image_preprocess import canny_frames
    frames = view_cases.frames(case)
    idx = canny_frames(len(frames))
    var = canny_cpu.frame_var(frames)
    if idx is None:
        return view_cases.digest(var), None, None
    return view_cases.digest(var), view_cases.digest(canny_cpu.canny_count(frames, idx)), len(idx)


def generate():
    image_process = load_image_process()
    records = []
    for case in view_cases.cases():
        changed, boxes = run_case(case, image_process)
        var_d, count_d, m = maps(case)
        records.append(dict(case, frames_digest=view_cases.digest(view_cases.frames(case)), changed=changed, boxes=boxes,
                            var_digest=var_d, count_digest=count_d, m=m))
    return dict(reference=PREP_SRC, reference_sha256=PREP_SHA256, numpy=np.__version__,
                canny="tests/canny_cpu.py (restated OpenCV 4.x non-IPP Canny, not pinned against cv2)", cases=records)


def dumps(doc):
    return json.dumps(doc, indent=None, separators=(",", ":"), sort_keys=False).replace('{"name"', '\n{"name"') + "\n"


def main(argv):
    doc = generate()
    text = dumps(doc)
    if "--check" in argv:
        with open(OUT) as f:
            same = f.read() == text
        print("view_preprocess.json reproduced" if same else "view_preprocess.json DIFFERS from the regenerated fixture")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    n_changed = sum(c["changed"] for c in doc["cases"])
    print(f"{OUT}: {len(doc['cases'])} cases, {n_changed} changed, {os.path.getsize(OUT) / 1024:.1f} KiB")
    for c in doc["cases"]:
        print(f"  {c['name']:28s} n={c['n']:3d} {c['size']} changed={c['changed']} boxes={c['boxes']}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
