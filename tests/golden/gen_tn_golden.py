"""Fixture of the temporal-network (TN) alignment, pinned on the reference (build container only):

    VSC_RUN_REFERENCE_CODE=1 python tests/golden/gen_tn_golden.py [--check]

The reference's `tn` and `iou` (VCSL, infer/vcsl/vta.py:80-95 and :244-363) are read from /root/reference at run time:
the file is pinned by SHA-256, parsed, and only those two function definitions are executed, in a namespace that holds
numpy, networkx and `dag_longest_path` -- nothing of the file's header runs (no loguru, numba, tslearn or torch import),
and no reference text is written anywhere.  The matrices come from tests/tn_cases.py; the fixture
(tests/golden/tn_align.json) stores their recipes and digests, the TN parameters and the reference's boxes, no matrices.

One deliberate deviation: inside that namespace `np.argsort` sorts with kind="stable".  The reference calls numpy's
default sort, which leaves the order of equal values unspecified, and that order changes the boxes when a row holds exact
ties (identical frames give identical descriptors).  This project fixes the rule -- descending similarity, ties to the
lower column -- and every case records whether the default sort would have given other boxes (`default_sort_differs`).
`--check` regenerates in memory and compares with the committed file instead of writing it.
"""
import ast
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tn_cases  # noqa: E402

REFERENCE = "/root/reference"
VTA_SRC = "VSC22-Descriptor-Track-1st/infer/vcsl/vta.py"
VTA_SHA256 = "1a86a766f183f1de7d749f2d2fc0cfffe0d923e8058fe36d0bd8da1748283418"
OPT_IN = "VSC_RUN_REFERENCE_CODE"
OUT = os.path.join(HERE, "tn_align.json")


class _NumpyStableArgsort:
    """numpy as the reference code sees it, except that argsort is stable (ties keep ascending index order)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, axis=-1, kind=None, order=None):
        return np.argsort(a, axis=axis, kind="stable", order=order)


def load_tn(stable=True):
    """-> (tn, iou) executed from the pinned vta.py; `stable=False` keeps numpy's default argsort."""
    if os.environ.get(OPT_IN) != "1":
        raise RuntimeError(f"executing reference code is opt-in: set {OPT_IN}=1")
    import networkx as nx
    from networkx.algorithms.dag import dag_longest_path
    path = os.path.join(REFERENCE, VTA_SRC)
    with open(path, "rb") as f:
        raw = f.read()
    if hashlib.sha256(raw).hexdigest() != VTA_SHA256:
        raise RuntimeError(f"{VTA_SRC} does not match its pinned SHA-256")
    tree = ast.parse(raw.decode("utf-8"), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in ("tn", "iou")]
    if sorted(d.name for d in defs) != ["iou", "tn"]:
        raise RuntimeError("tn / iou definitions not found")
    ns = {"np": _NumpyStableArgsort() if stable else np, "nx": nx, "dag_longest_path": dag_longest_path,
          "List": list, "Tuple": tuple, "Any": object}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns["tn"], ns["iou"]


def run_case(case, tn):
    m = tn_cases.matrix(case)
    sims = m + case["bias"]           # VCSLLocalization.similarity_all: the fp32 matrix plus the Python-float bias
    with np.errstate(divide="ignore", invalid="ignore"):
        return [[int(v) for v in box] for box in tn(sims, **case["params"])]


def generate():
    import networkx as nx
    tn_stable, _ = load_tn(stable=True)
    tn_default, _ = load_tn(stable=False)
    records = []
    for case in tn_cases.cases():
        boxes = run_case(case, tn_stable)
        records.append(dict(case, digest=tn_cases.digest(tn_cases.matrix(case)), boxes=boxes,
                            default_sort_differs=run_case(case, tn_default) != boxes))
    return dict(reference=VTA_SRC, reference_sha256=VTA_SHA256, numpy=np.__version__, networkx=nx.__version__,
                argsort="stable (descending similarity, ties to the lower column)", cases=records)


def dumps(doc):
    return json.dumps(doc, indent=None, separators=(",", ":"), sort_keys=False).replace('{"name"', '\n{"name"') + "\n"


def main(argv):
    doc = generate()
    text = dumps(doc)
    if "--check" in argv:
        with open(OUT) as f:
            same = f.read() == text
        print("tn_align.json reproduced" if same else "tn_align.json DIFFERS from the regenerated fixture")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    n_boxes = sum(len(c["boxes"]) for c in doc["cases"])
    n_diff = sum(c["default_sort_differs"] for c in doc["cases"])
    print(f"{OUT}: {len(doc['cases'])} cases, {n_boxes} boxes, default argsort differs in {n_diff}, "
          f"{os.path.getsize(OUT) / 1024:.1f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
