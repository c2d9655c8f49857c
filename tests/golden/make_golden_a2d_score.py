"""Generates tests/golden/a2d_score_cases.npz: the synthetic scoring cases of tests/_a2d_score.py (make_cases) as run-length
strings, and per case the tuple the reference's own calculate_precision_at_k_and_iou_metrics (datasets/a2d_eval.py:20-45) returns
for them (build machine only).

a2d_eval.py is loaded by file path (importlib), not through the reference's `datasets` package.  It imports pycocotools, which is
absent, so this maker installs its own stand-ins first: a `pycocotools.coco` whose COCO is an empty class, and a `pycocotools.mask`
whose `decode` is the plain-loop restatement of cocoapi's rleFrString + rleDecode (tests/_a2d.py).  The ground truth and the
predictions are two such COCO instances with .imgs and .imgToAnns filled in.  So the choice of the prediction, compute_iou, the
thresholds and the sums are the reference's own code; the decoding is the restatement's, not pycocotools' C code.

Mask AP is NOT in this file's reference part and is not verified against pycocotools anywhere: pycocotools is on no machine this
project can use.  The tests hold a2d_score.coco_mask_ap to the plain-loop restatement of COCOeval in tests/_a2d_score.py and to
cases derived by hand.

Run from the repository root:  python tests/golden/make_golden_a2d_score.py
The file it writes is data.  names: the case names; per case X with K images of N predictions each:
  X_image_ids [K] i64, X_sizes [K,2] i64, X_areas [K] f64 (NaN: the annotation carries no area), X_scores [K,N] f64
  X_gt uint8, X_gt_ends [K]          the K ground-truth count strings, concatenated, and where each ends
  X_pred uint8, X_pred_ends [K*N]    the K*N prediction count strings likewise, image after image
  X_precision [5] f64, X_overall_iou, X_mean_iou f64     the reference's tuple
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _a2d  # noqa: E402
import _a2d_score as S  # noqa: E402

REF_ROOT = os.environ.get("TCE_REFERENCE_ROOT", "/root/reference")


def load_reference_eval():
    class COCO:
        pass

    pc, coco, mask = types.ModuleType("pycocotools"), types.ModuleType("pycocotools.coco"), types.ModuleType("pycocotools.mask")
    coco.COCO = COCO
    mask.decode = lambda seg: _a2d.rle_decode(_a2d.rle_from_string(seg["counts"]), int(seg["size"][0]), int(seg["size"][1]))
    pc.coco, pc.mask = coco, mask
    sys.modules.update({"pycocotools": pc, "pycocotools.coco": coco, "pycocotools.mask": mask})
    spec = importlib.util.spec_from_file_location("ref_a2d_eval", os.path.join(REF_ROOT, "datasets", "a2d_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, COCO


def main():
    ref, COCO = load_reference_eval()
    out = {"names": []}
    for name, images in S.make_cases().items():
        gts = [S.encode(im["gt"]) for im in images]
        prs = [S.encode(p) for im in images for p in im["preds"]]
        N = len(images[0]["preds"])
        coco_gt, coco_pred = COCO(), COCO()
        coco_gt.imgs = {im["image_id"]: {"id": im["image_id"]} for im in images}
        coco_gt.imgToAnns = {im["image_id"]: [{"segmentation": {"size": list(im["size"]), "counts": g}}] for im, g in zip(images, gts)}
        coco_pred.imgToAnns = {im["image_id"]: [{"segmentation": {"size": list(im["size"]), "counts": prs[k * N + n]}, "score": float(im["scores"][n])}
                                                for n in range(N)] for k, im in enumerate(images)}
        precision, overall_iou, mean_iou = ref.calculate_precision_at_k_and_iou_metrics(coco_gt, coco_pred)
        out["names"].append(name)
        out[f"{name}_image_ids"] = np.asarray([im["image_id"] for im in images], dtype=np.int64)
        out[f"{name}_sizes"] = np.asarray([im["size"] for im in images], dtype=np.int64)
        out[f"{name}_areas"] = np.asarray([np.nan if im["area"] is None else im["area"] for im in images], dtype=np.float64)
        out[f"{name}_scores"] = np.asarray([im["scores"] for im in images], dtype=np.float64)
        out[f"{name}_gt"], out[f"{name}_gt_ends"] = np.frombuffer(b"".join(gts), dtype=np.uint8), np.cumsum([len(g) for g in gts])
        out[f"{name}_pred"], out[f"{name}_pred_ends"] = np.frombuffer(b"".join(prs), dtype=np.uint8), np.cumsum([len(p) for p in prs])
        out[f"{name}_precision"] = np.asarray(precision, dtype=np.float64)
        out[f"{name}_overall_iou"], out[f"{name}_mean_iou"] = np.float64(overall_iou), np.float64(mean_iou)
        per = S.per_image_of([{"image_id": im["image_id"], "size": im["size"], "gt": g, "preds": prs[k * N:(k + 1) * N], "scores": im["scores"],
                               "area": im["area"]} for k, (im, g) in enumerate(zip(images, gts))])
        print(f"{name}: {len(images)} images x {N}: P@K {np.asarray(precision).tolist()} overall {overall_iou:.6f} mean {mean_iou:.6f}; "
              f"AP (restatement, not pycocotools) {[round(v, 4) for v in S.coco_mask_ap_loops(per)]}")
    out["names"] = np.asarray(out["names"])
    path = os.path.join(HERE, "a2d_score_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
