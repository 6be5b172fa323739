"""Fixture of the DP and HV temporal alignments, pinned on the reference (build container only):

    VSC_RUN_REFERENCE_CODE=1 python tests/golden/gen_align_golden.py [--check]

The reference's `iou`, `zero_runs`, `cut_path`, `find_path`, `njit_dp_matrix`, `dp` and `hv` (VCSL, infer/vcsl/vta.py:80-127,
:153-241 and :366-426) are read from /root/reference at run time: the file is pinned by SHA-256, parsed, and only those
function definitions are executed, in a namespace that holds numpy and stand-ins for what the file's header would import --
`njit` returns the function undecorated, `prange` is `range`, and the numpy the code sees adds `NINF` (gone in numpy 2).
Nothing of the header runs (no loguru, numba, tslearn or torch import) and no reference text is written anywhere.  The
matrices come from tests/align_cases.py; the fixture (tests/golden/align_dp_hv.json) stores their recipes and digests, the
parameters and the reference's boxes, no matrices.

Run undecorated under numpy 2, `njit_dp_matrix` computes in float32 throughout; that is the contract of the kernels.  Under
numba's typing its two half-weight candidates and the `min_sim` comparison are float64; each DP case records whether that
would change the boxes (`wide_differs`, from tests/align_contract.py with wide=True).  `--check` regenerates in memory and
compares with the committed file instead of writing it.
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

import align_cases  # noqa: E402
import align_contract  # noqa: E402

REFERENCE = "/root/reference"
VTA_SRC = "VSC22-Descriptor-Track-1st/infer/vcsl/vta.py"
VTA_SHA256 = "1a86a766f183f1de7d749f2d2fc0cfffe0d923e8058fe36d0bd8da1748283418"
OPT_IN = "VSC_RUN_REFERENCE_CODE"
OUT = os.path.join(HERE, "align_dp_hv.json")
NAMES = ("iou", "zero_runs", "cut_path", "find_path", "njit_dp_matrix", "dp", "hv")


class _NumpyWithNinf:
    """numpy as the reference code sees it, plus the `NINF` alias that numpy 2 removed."""
    NINF = -np.inf

    def __getattr__(self, name):
        return getattr(np, name)


def load_reference():
    """-> {name: function} executed from the pinned vta.py."""
    if os.environ.get(OPT_IN) != "1":
        raise RuntimeError(f"executing reference code is opt-in: set {OPT_IN}=1")
    path = os.path.join(REFERENCE, VTA_SRC)
    with open(path, "rb") as f:
        raw = f.read()
    if hashlib.sha256(raw).hexdigest() != VTA_SHA256:
        raise RuntimeError(f"{VTA_SRC} does not match its pinned SHA-256")
    tree = ast.parse(raw.decode("utf-8"), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in NAMES]
    if sorted(d.name for d in defs) != sorted(NAMES):
        raise RuntimeError("the DP / HV function definitions were not found")
    ns = {"np": _NumpyWithNinf(), "njit": lambda: (lambda f: f), "prange": range, "List": list, "Tuple": tuple, "Any": object}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return {n: ns[n] for n in NAMES}


def run_case(case, ref):
    m = align_cases.matrix(case)
    sims = m + case["bias"]           # VCSLLocalization.similarity_all: the fp32 matrix plus the Python-float bias (a new array:
    fn = ref["dp"] if case["model"] == "DP" else ref["hv"]           # both functions write into their argument)
    with np.errstate(divide="ignore", invalid="ignore"):
        return [[int(v) for v in box] for box in fn(sims, **case["params"])]


def generate():
    ref = load_reference()
    records = []
    for case in align_cases.cases():
        m = align_cases.matrix(case)
        rec = dict(case, digest=align_cases.digest(m), boxes=run_case(case, ref))
        if case["model"] == "DP":
            rec["wide_differs"] = align_contract.dp_contract(m, case["bias"], wide=True, **case["params"])[0] != rec["boxes"]
        records.append(rec)
    return dict(reference=VTA_SRC, reference_sha256=VTA_SHA256, numpy=np.__version__,
                typing="numpy 2 scalar rules: float32 throughout (wide_differs: numba's float64 half-weight candidates)",
                cases=records)


def dumps(doc):
    return json.dumps(doc, indent=None, separators=(",", ":"), sort_keys=False).replace('{"name"', '\n{"name"') + "\n"


def main(argv):
    doc = generate()
    text = dumps(doc)
    if "--check" in argv:
        with open(OUT) as f:
            same = f.read() == text
        print("align_dp_hv.json reproduced" if same else "align_dp_hv.json DIFFERS from the regenerated fixture")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    for model in ("DP", "HV"):
        own = [c for c in doc["cases"] if c["model"] == model]
        print(f"{model}: {len(own)} cases, {sum(len(c['boxes']) for c in own)} boxes, "
              f"wide differs in {sum(c.get('wide_differs', False) for c in own)}")
    print(f"{OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
