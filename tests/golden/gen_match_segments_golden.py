"""Fixture of the segment extraction (connected components + RANSAC), pinned on the reference (build container only):

    VSC_RUN_REFERENCE_CODE=1 python tests/golden/gen_match_segments_golden.py [--check]

The reference's `generate_matching_result` (VSC22-Matching-Track-1st/infer/src/utils.py:76-117) is read from
/root/reference at run time: the file is pinned by SHA-256, parsed, and only that function definition is executed, in a
namespace that holds numpy, sklearn's RANSACRegressor and two stated stand-ins -- nothing of the file's header runs and no
reference text is written anywhere.  Stand-ins: `cv2.connectedComponentsWithStats` is scipy.ndimage.label with the 3 x 3
structure (cv2 is not a dependency; the labelling ORDER may differ from cv2's, the components do not, and rows are
compared as sorted sets); `tqdm.tqdm` is the identity.  The result is asserted equal to oracle.matching_oracle.matching_result.

The maps come from tests/seg_cases.py; the fixture (tests/golden/match_segments.json) stores their recipes and digests,
the three (threshold, std_ratio) passes, and per (case, pass) the reference rows, the contract's margin and the tier:

  A  the contract (tests/seg_contract.py) met no boundary point in any executed trial
  B  not A, but the reference code gives the same endpoints with residual_threshold 2 - 1e-9, 2 and 2 + 1e-9 ("twin-robust")
  C  the rest: sklearn's own answer is decided by rounding noise

plus whether the contract's endpoints equal the reference's and the largest score difference.  No matrices are stored.
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
sys.path.insert(0, ROOT)

import seg_cases  # noqa: E402
import seg_contract  # noqa: E402

REFERENCE = "/root/reference"
UTILS_SRC = "VSC22-Matching-Track-1st/infer/src/utils.py"
UTILS_SHA256 = "80423b34cdda6caeb06b4f53673589e9457a8250feca7af8d0b9c8ca207e5ffd"
OPT_IN = "VSC_RUN_REFERENCE_CODE"
OUT = os.path.join(HERE, "match_segments.json")
TWIN_DELTA = 1e-9

# conditions on the fixture (asserted, not measured)
MIN_ENTRIES, MAX_TIER_C, MIN_TIER_A, MIN_SEGMENTS_AB, MAX_KNIFE_EDGE = 150, 0.25, 40, 150, 0.02


class _Cv2:
    @staticmethod
    def connectedComponentsWithStats(binary, connectivity=8):
        from scipy import ndimage
        assert connectivity == 8
        labels, count = ndimage.label(binary > 0, structure=np.ones((3, 3), dtype=np.int32))
        return count + 1, labels.astype(np.int32), None, None


class _Tqdm:
    @staticmethod
    def tqdm(it):
        return it


def load_reference(delta=0.0):
    """-> generate_matching_result executed from the pinned utils.py; `delta` is added to the residual threshold."""
    if os.environ.get(OPT_IN) != "1":
        raise RuntimeError(f"executing reference code is opt-in: set {OPT_IN}=1")
    from sklearn.linear_model import RANSACRegressor
    path = os.path.join(REFERENCE, UTILS_SRC)
    with open(path, "rb") as f:
        raw = f.read()
    if hashlib.sha256(raw).hexdigest() != UTILS_SHA256:
        raise RuntimeError(f"{UTILS_SRC} does not match its pinned SHA-256")
    tree = ast.parse(raw.decode("utf-8"), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "generate_matching_result"]
    if len(defs) != 1:
        raise RuntimeError("generate_matching_result not found")

    def ransac(**kw):
        kw["residual_threshold"] = kw["residual_threshold"] + delta
        return RANSACRegressor(**kw)

    ns = {"np": np, "cv2": _Cv2, "tqdm": _Tqdm, "RANSACRegressor": ransac}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns["generate_matching_result"]


def _rows(res):
    """rows of one map -> sorted [[x_first, y_first, x_last, y_last, score], ...]"""
    return sorted([[int(r[2]), int(r[3]), int(r[4]), int(r[5]), float(r[6])] for r in res])


def _ends(rows):
    return [r[:4] for r in rows]


def generate():
    import scipy
    import sklearn
    from oracle import matching_oracle
    ref, ref_lo, ref_hi = load_reference(), load_reference(-TWIN_DELTA), load_reference(TWIN_DELTA)
    records = []
    tiers = {"A": 0, "B": 0, "C": 0}
    score_diff = {"A": 0.0, "B": 0.0, "C": 0.0}
    ends_equal = {"A": [0, 0], "B": [0, 0], "C": [0, 0]}
    knife, segments_ab, entries = 0, 0, 0
    for case in seg_cases.cases():
        m = seg_cases.matrix(case)
        item = [["Q", "R", m, None]]
        passes = []
        for threshold, std_ratio in seg_cases.PASSES:
            want = _rows(ref(item, threshold=threshold, std_ratio=std_ratio))
            oracle_rows = _rows(matching_oracle.matching_result(item, threshold, std_ratio))
            assert _ends(oracle_rows) == _ends(want) and np.allclose([r[4] for r in oracle_rows], [r[4] for r in want], rtol=0, atol=1e-12), \
                (case["name"], threshold)
            got, report = seg_contract.segments(m, threshold, std_ratio)
            got = sorted(got)
            robust = _ends(_rows(ref_lo(item, threshold=threshold, std_ratio=std_ratio))) == _ends(want) == \
                _ends(_rows(ref_hi(item, threshold=threshold, std_ratio=std_ratio)))
            tier = "A" if not report["boundary"] else ("B" if robust else "C")
            same = _ends(got) == _ends(want)
            diff = max([abs(a[4] - b[4]) for a, b in zip(got, want)], default=0.0) if same else None
            entries += 1
            tiers[tier] += 1
            ends_equal[tier][0] += same
            ends_equal[tier][1] += 1
            if same:
                score_diff[tier] = max(score_diff[tier], diff)
            if tier in "AB":
                segments_ab += len(want)
            margin = report["margin"]
            knife += margin < seg_contract.KNIFE_EDGE
            passes.append(dict(threshold=threshold, std_ratio=std_ratio, tier=tier, rows=want,
                               margin=None if margin == float("inf") else margin, endpoints_equal=same, score_diff=diff,
                               group_sizes=report["group_sizes"]))
        records.append(dict(case, digest=seg_cases.digest(m), passes=passes))
    summary = dict(entries=entries, tiers=tiers, endpoints_equal={t: f"{a} of {b}" for t, (a, b) in ends_equal.items()},
                   max_score_diff=score_diff, segments_in_tiers_ab=segments_ab, knife_edges=knife)
    assert entries >= MIN_ENTRIES, summary
    assert tiers["C"] <= MAX_TIER_C * entries, summary
    assert tiers["A"] >= MIN_TIER_A, summary
    assert segments_ab >= MIN_SEGMENTS_AB, summary
    assert knife <= MAX_KNIFE_EDGE * entries, summary
    return dict(reference=UTILS_SRC, reference_sha256=UTILS_SHA256, numpy=np.__version__, scipy=scipy.__version__,
                sklearn=sklearn.__version__, stand_ins="cv2.connectedComponentsWithStats -> scipy.ndimage.label (3x3), tqdm -> identity",
                passes=[list(p) for p in seg_cases.PASSES], twin_delta=TWIN_DELTA, knife_edge=seg_contract.KNIFE_EDGE,
                summary=summary, cases=records)


def dumps(doc):
    return json.dumps(doc, indent=None, separators=(",", ":"), sort_keys=False).replace('{"name"', '\n{"name"') + "\n"


def main(argv):
    doc = generate()
    text = dumps(doc)
    if "--check" in argv:
        with open(OUT) as f:
            same = f.read() == text
        print("match_segments.json reproduced" if same else "match_segments.json DIFFERS from the regenerated fixture")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{OUT}: {json.dumps(doc['summary'])}, {os.path.getsize(OUT) / 1024:.1f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
