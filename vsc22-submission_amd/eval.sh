#!/bin/bash
# Candidate generation (+ localisation when the reference's vcsl package is importable) and, with GT=<matches csv>, the descriptor-track
# uAP (stands where the reference's infer/eval.sh stands).  ALIGNMENT=hip writes matches.csv with the HIP TN kernel instead of VCSL;
# ALIGNMENT_MODEL=DP / HV picks VCSL's DP or HV model instead of TN (on the device too with ALIGNMENT=hip);
# CANDIDATES=hip cuts the global top-k and groups it into video pairs on the device (the same candidates.csv);
# SEGMENT_METRIC=hip scores matches.csv against GT by the matching-track segment AP on the device ("Matching track metric");
# UAP=hip computes the uAP itself on the device, in the reference's summation order.
set -e
cd "$(dirname "$0")"
export PYTHONPATH=$PYTHONPATH:$PWD
OUT=${OUT:-./outputs}; SPLIT=${SPLIT:-test}
python -m vsc.baseline.sscd_baseline --query_features "$OUT/${SPLIT}_query_sn.npz" --ref_features "$OUT/${SPLIT}_refs_sn.npz" \
  --output_path "$OUT/" --overwrite --alignment "${ALIGNMENT:-vcsl}" --alignment_model "${ALIGNMENT_MODEL:-TN}" --candidates "${CANDIDATES:-host}" --segment_metric "${SEGMENT_METRIC:-none}" --uap "${UAP:-host}" ${GT:+--ground_truth "$GT"}
