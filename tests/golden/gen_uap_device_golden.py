"""Generates tests/golden/uap_device.json: what the REFERENCE's own vsc.metrics.average_precision
(VSC22-Descriptor-Track-1st/infer/vsc/metrics.py:423-494, with the sklearn / numpy / pandas installed beside it) returns on every
case of tests/uap_cases.py -- `.ap`, `.simple_ap` and the curve as uint64 bit patterns, the number of correct predictions, or the
type of the exception it raises.  The curve is stored in full up to 300 predictions and as the SHA-256 of its bytes (precisions,
recalls, scores, float64 each) above.  Only results are stored: the cases are rebuilt from their seeds, and none of the
reference's text is copied.  Build container only; opt-in like every helper that executes the reference (VSC_RUN_REFERENCE_CODE=1).
The reference file is imported as a module, as gen_uap_golden.py does: tests/golden/_reference_classes.load_definitions pins a file
list and an import whitelist that hold neither this file nor pandas / sklearn.

    VSC_RUN_REFERENCE_CODE=1 python tests/golden/gen_uap_device_golden.py
"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/VSC22-Descriptor-Track-1st/infer/vsc/metrics.py"
OUT = os.path.join(HERE, "uap_device.json")
FULL_CURVE_MAX = 300
sys.path.insert(0, os.path.dirname(HERE))


def load_reference():
    if os.environ.get("VSC_RUN_REFERENCE_CODE") != "1":
        raise RuntimeError("executing the reference is opt-in: set VSC_RUN_REFERENCE_CODE=1")
    spec = importlib.util.spec_from_file_location("ref_vsc_metrics", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def u64(values):
    return np.ascontiguousarray(values, np.float64).view(np.uint64).tolist()


def main():
    import uap_cases
    ref = load_reference()
    import pandas
    import sklearn
    out = {"versions": {"numpy": np.__version__, "pandas": pandas.__version__, "sklearn": sklearn.__version__}, "cases": {}}
    for case in uap_cases.cases():
        gt, preds = uap_cases.pairs(case, ref.CandidatePair)
        rec = {"n": len(preds), "g": len(gt)}
        try:
            ap = ref.average_precision(gt, preds)
        except Exception as e:      # noqa: BLE001 -- the type is the datum
            rec["raises"] = type(e).__name__
            rec["message"] = str(e)[:80]
        else:
            c = ap.pr_curve
            rec["ap"], rec["simple_ap"] = u64([ap.ap])[0], u64([ap.simple_ap])[0]
            rec["n_pos"] = len(c.precisions)
            rows = [np.ascontiguousarray(v, np.float64) for v in (c.precisions, c.recalls, c.scores)]
            if len(preds) <= FULL_CURVE_MAX:
                rec["curve"] = [u64(v) for v in rows]
            else:
                rec["curve_sha256"] = hashlib.sha256(b"".join(v.tobytes() for v in rows)).hexdigest()
        print(case["name"], rec["n"], rec["g"], rec.get("raises") or (float(ap.ap), float(ap.simple_ap), rec["n_pos"]))
        out["cases"][case["name"]] = rec
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
