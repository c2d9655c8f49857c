"""Generates tests/golden/a2d_post_cases.npz: the reference's own A2DSentencesPostProcess (models/postprocessors.py:14-54) run on
the CPU on the cases of tests/_a2d.py (build machine only; the reference is imported through ref_harness).

pycocotools is absent, and ref_harness installs an empty `pycocotools.mask` stand-in: this maker sets its `encode` to the plain-loop
restatement of cocoapi's rleEncode + rleToString (tests/_a2d.py: encode).  So masks and scores are the reference class's own
output, and the strings are produced at the reference's own call site, with its own Fortran-order handling -- but by the
restatement, not by pycocotools' C code.

Run from the repository root:  python tests/golden/make_golden_a2d.py
The file it writes is data.  Per case X of tests/_a2d.py CASES (A, B, C, D):
  X_logits [N] f32, X_masks [N,h,w] f32     inputs (torch.Generator(seed))
  X_size [2], X_orig [2]                    the un-padded model-input size and the dataset's frame size
  X_scores [N] f32                          the class's scores
  X_ref                                     np.packbits of the class's masks [N,H0,W0] (float 0/1 planes there)
  X_contested                               np.packbits of the bool [N,H0,W0] mask of pixels whose bit hangs on rounding
  X_rle uint8, X_rle_ends [N]               the N count strings of rle_masks, concatenated, and where each ends
names: the case names in order.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _a2d  # noqa: E402
import ref_harness  # noqa: E402


def main():
    ref_harness.import_reference()
    import pycocotools.mask as mask_util
    mask_util.encode = _a2d.encode
    from models.postprocessors import A2DSentencesPostProcess
    post = A2DSentencesPostProcess(threshold=0.5)
    out = {"names": np.asarray([c[0] for c in _a2d.CASES])}
    for name, seed, N, hw, size, orig, kind, scale in _a2d.CASES:
        logits, masks = _a2d.make_inputs(seed, N, hw, kind, scale)
        outputs = {"pred_logits": logits.view(1, 1, N, 1), "pred_masks": masks.view(1, 1, N, *hw)}
        res = post(outputs, torch.tensor([orig]), torch.tensor([size]))
        assert len(res) == 1
        ref = res[0]["masks"][:, 0]
        assert tuple(ref.shape) == (N,) + tuple(orig) and bool(((ref == 0) | (ref == 1)).all())
        mine, v = _a2d.reference_post(masks, size, orig)
        assert torch.equal(mine, ref.to(torch.uint8)), "the restatement is not the class"
        cont = _a2d.contested(v)
        share = float(cont.float().mean())
        rle = [r["counts"] for r in res[0]["rle_masks"]]
        for n in range(N):
            assert res[0]["rle_masks"][n]["size"] == list(orig)
            assert np.array_equal(_a2d.rle_decode(_a2d.rle_from_string(rle[n]), *orig), ref[n].numpy().astype(np.uint8))
        out[f"{name}_logits"], out[f"{name}_masks"] = logits.numpy(), masks.numpy()
        out[f"{name}_size"], out[f"{name}_orig"] = np.asarray(size), np.asarray(orig)
        out[f"{name}_scores"] = res[0]["scores"].numpy()
        out[f"{name}_ref"] = np.packbits(ref.numpy().astype(np.uint8))
        out[f"{name}_contested"] = np.packbits(cont.numpy())
        out[f"{name}_rle"] = np.frombuffer(b"".join(rle), dtype=np.uint8)
        out[f"{name}_rle_ends"] = np.cumsum([len(r) for r in rle])
        runs = [len(_a2d.rle_from_string(r)) for r in rle]
        print(f"{name}: N={N} masks {tuple(ref.shape)} contested share {share:.3e} ones {float(ref.mean()):.3f} runs per mask {runs} "
              f"max |v| {float(v.abs().max()):.1f}")
        if name in ("C", "D"):
            assert share == 0.0, f"case {name} must have no contested pixel: its strings are compared byte for byte"
        assert share <= _a2d.MAX_SHARE
    path = os.path.join(HERE, "a2d_post_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
