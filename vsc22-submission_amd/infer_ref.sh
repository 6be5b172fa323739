#!/bin/bash
# Reference-side extraction of the ensemble, one process per GPU (stands where the reference's infer/infer_ref.sh stands):
# every backbone over the train and test reference videos, then concat + PCA + score normalisation.
# RESIZE=hip resizes the decoded frames to the encoders' inputs on the GPU instead of with Pillow in the loader workers (the same files).
# DECODE_SPLIT=markers|substreams|all (with DECODE=hip) decodes in parallel inside a frame.
# DECODE_SCANS=hip (with DECODE=hip) decodes progressive and other multi-scan jpgs on the GPU too.
# DECODE=hip (with RESIZE=hip) decodes the jpgs on the GPU too: the workers hand the compressed files on (the same files).
#   CKPT=../checkpoints ZIPS=../data/jpg_zips META=../data/meta bash infer_ref.sh
set -e
cd "$(dirname "$0")"
export PYTHONPATH=$PYTHONPATH:$PWD
CKPT=${CKPT:-../checkpoints}; ZIPS=${ZIPS:-../data/jpg_zips}; META=${META:-../data/meta}; OUT=${OUT:-./outputs}
GPUS=${GPUS:-$(rocm-smi --showid 2>/dev/null | grep -c "GPU\[" || echo 1)}; [ "$GPUS" -ge 1 ] || GPUS=1
PRECISION=${PRECISION:-fp16}     # MFMA operand type of the encoders; bf16 = the benchmarked configuration
# name : preset : weight naming  (the reference's four descriptor models, infer_ref.sh:7-8)
MODELS=("swinv2_v115:swinv2_base_256:swin_ref" "swinv2_v107:swinv2_base_256:swin_ref" "swinv2_v106:swinv2_base_256:swin_ref" "vit_v68:vit_v68:timm_vit")
for m in "${MODELS[@]}"; do
  IFS=: read -r name arch fmt <<< "$m"
  mkdir -p "$OUT/$name"
  for split in train test; do
    python -m torch.distributed.run --nnodes=1 --nproc-per-node "$GPUS" --master-addr 127.0.0.1 extract_ref_feats.py \
      --zip_prefix "$ZIPS" --input_file "$META/$split/${split}_ref_vids.txt" --save_file "$OUT/$name/${split}_refs" \
      --checkpoint_path "$CKPT/$name.torchscript.pt" --arch "$arch" --weights_format "$fmt" --batch_size 2 --precision "$PRECISION" \
      --resize "${RESIZE:-host}" --decode "${DECODE:-host}" --decode_split "${DECODE_SPLIT:-none}" --decode_scans "${DECODE_SCANS:-host}"
  done
done
# PCA_FIT=hip fits the PCA on the train references on the GPU (implies --fit_pca; the model file is then an .npz, read by infer_query.sh
# through the same PCA_MODEL); FIT_PCA=1 alone fits with sklearn on the host as the reference does and pickles it
if [ "${PCA_FIT:-sklearn}" = hip ]; then PCA_MODEL=${PCA_MODEL:-$CKPT/pca_model.npz}; FIT_ARGS="--fit_pca --pca_fit hip"; else PCA_MODEL=${PCA_MODEL:-$CKPT/pca_model.pkl}; FIT_ARGS=${FIT_PCA:+--fit_pca}; fi
# SCORE_NORM=hip runs the score normalisation of the two merged sets on the GPU (one upload per set; the same <set>_sn.npz)
python concat_pca_sn.py --root "$OUT" --models swinv2_v115 swinv2_v107 swinv2_v106 vit_v68 --pca_model "$PCA_MODEL" $FIT_ARGS \
  --score_norm "${SCORE_NORM:-host}"
