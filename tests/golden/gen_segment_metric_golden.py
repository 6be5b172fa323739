"""Generates tests/golden/segment_metric.json: the cases of tests/segment_metric_cases.py and what the REFERENCE's own
match_metric (/root/reference/VSC22-Matching-Track-1st/infer/vsc/metrics.py:309-383) returns on them -- `.ap` and every value of
the precision / recall curve as float.hex(), or the ZeroDivisionError it raises.  Build container only (imports the reference
file); the json travels.

    python tests/golden/gen_segment_metric_golden.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/VSC22-Matching-Track-1st/infer/vsc/metrics.py"
OUT = os.path.join(HERE, "segment_metric.json")
sys.path.insert(0, os.path.dirname(HERE))


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_vsc_matching_metrics", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import segment_metric_cases
    ref = load_reference()
    out = []
    for name, gts, preds in segment_metric_cases.cases():
        G = [ref.Match(q, r, 1.0, *box) for q, r, *box in gts]
        P = [ref.Match(q, r, s, *box) for q, r, s, *box in preds]
        rec = {"name": name, "gts": [list(g) for g in gts], "preds": [list(p) for p in preds]}
        try:
            ap = ref.match_metric(G, P)
        except ZeroDivisionError:
            rec["raises"] = "ZeroDivisionError"
        else:
            rec["ap"] = float(ap.ap).hex()
            for field in ("precisions", "recalls", "scores"):
                rec[field] = [float(v).hex() for v in getattr(ap.pr_curve, field)]
        print(name, len(gts), len(preds), rec.get("raises") or (float.fromhex(rec["ap"]), len(rec["recalls"])))
        out.append(rec)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
