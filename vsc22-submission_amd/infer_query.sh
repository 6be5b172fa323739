#!/bin/bash
# Query-side extraction (stands where the reference's infer/infer_query.sh stands): ensemble + video-score gate + de-duplication + PCA +
# query score normalisation, per split.  PREPROCESS=hip crops static borders and splits stacked views on the GPU first (the reference's
# image_process); the default, none, encodes whole frames.  SCORE_NORM=hip runs the query score normalisation on the GPU (the same file).
# VIEW_DECISIONS=hip (with PREPROCESS=hip) takes the border / split decisions on the GPU too: only the boxes come back (the same files).
# FRAME_FILTER=hip runs the near-duplicate frame filter on the GPU (the same files wherever a video's frame means are pairwise distinct).
# RESIZE=hip makes every encoder input and the video-score input from the decoded frames on the GPU instead of with Pillow in the
# loader workers, with or without PREPROCESS=hip (the same files).  DECODE_SPLIT=markers|substreams|all (with DECODE=hip) decodes in parallel inside a frame.  DECODE=hip (with RESIZE=hip) decodes the jpgs on the GPU too: the
# workers hand the compressed files on (the same files; a video with a frame that is no baseline JPEG is decoded by its worker).
#   CKPT=../checkpoints ZIPS=../data/jpg_zips META=../data/meta bash infer_query.sh
set -e
cd "$(dirname "$0")"
export PYTHONPATH=$PYTHONPATH:$PWD
CKPT=${CKPT:-../checkpoints}; ZIPS=${ZIPS:-../data/jpg_zips}; META=${META:-../data/meta}; OUT=${OUT:-./outputs}
PRECISION=${PRECISION:-fp16}
PCA_MODEL=${PCA_MODEL:-$CKPT/pca_model.pkl}    # after PCA_FIT=hip bash infer_ref.sh: PCA_MODEL=$CKPT/pca_model.npz
for split in ${SPLITS:-train val test}; do
  # the other split's references are the score-normalisation bank (extract_query_feats.py:47-50 of the reference)
  if [ "$split" = test ]; then NORM="$OUT/train_refs.npz"; else NORM="$OUT/test_refs.npz"; fi
  python extract_query_feats.py --split "$split" --precision "$PRECISION" \
    --models "swinv2_base_256:swin_ref:$CKPT/swinv2_v115.torchscript.pt" "swinv2_base_256:swin_ref:$CKPT/swinv2_v107.torchscript.pt" \
             "swinv2_base_256:swin_ref:$CKPT/swinv2_v106.torchscript.pt" "vit_v68:timm_vit:$CKPT/vit_v68.torchscript.pt" \
    --pca_model "$PCA_MODEL" --zip_prefix "$ZIPS" --input_file "$META/$split/${split}_query_ids.txt" --norm_refs "$NORM" \
    --clip_checkpoint "$CKPT/clip.torchscript.pt" --vsm_checkpoint "$CKPT/vsm.torchscript.pt" --output_dir "$OUT" \
    --preprocess "${PREPROCESS:-none}" --view_decisions "${VIEW_DECISIONS:-host}" --score_norm "${SCORE_NORM:-host}" \
    --frame_filter "${FRAME_FILTER:-host}" --resize "${RESIZE:-host}" --decode "${DECODE:-host}" --decode_split "${DECODE_SPLIT:-none}" --decode_scans "${DECODE_SCANS:-host}"
done
