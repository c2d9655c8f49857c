"""Generates tests/golden/davis_label_cases.npz: the Ref-DAVIS caller stage (inference_davis.py:239-248, 294-298) restated with the
same PyTorch primitives the driver uses (tests/_davis.py: reference_labels), on the CPU (build machine only).

Run from the repository root:  python tests/golden/make_golden_davis.py
The file it writes is data.  Per case X of tests/_davis.py CASES (A, B, D, E):
  X_logits [n,T,Q,1] f32                            inputs (torch.Generator(seed); D with its two saturated blocks)
  X_masks_bytes [4, n*T*Q*h*w] uint8, X_masks_shape   the fp32 masks [n,T,Q,h,w] as four byte planes (byte b of every value: the
                                                    exponent plane deflates, which keeps the file under 1 MB; _davis.load_cases
                                                    puts the same bits back together)
  X_size [2]                                        (H0, W0)
  X_best [n] int32                                  best query per object
  X_labels [T,H0,W0] uint8                          the driver's label map (0 = background, k + 1 = object k)
  X_contested                                       np.packbits of the bool [T,H0,W0] mask of pixels whose label hangs on rounding
names: the case names in order.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _davis  # noqa: E402


def main():
    out = {"names": np.asarray([c[0] for c in _davis.CASES])}
    for name, seed, n, T, Q, hw, size, scale in _davis.CASES:
        logits, masks = _davis.make_inputs(name, seed, n, T, Q, hw, scale)
        labels, best, contested = _davis.reference_labels(list(logits), list(masks), size)
        out[f"{name}_logits"] = logits.numpy()
        out[f"{name}_masks_bytes"] = np.ascontiguousarray(masks.numpy().view(np.uint8).reshape(-1, 4).T)
        out[f"{name}_masks_shape"] = np.asarray(masks.shape)
        out[f"{name}_size"] = np.asarray(size)
        out[f"{name}_best"], out[f"{name}_labels"] = best.numpy(), labels.numpy()
        out[f"{name}_contested"] = np.packbits(contested.numpy())
        ties = 0
        if name == "D":  # exact saturated ties: both blocks' objects at 1.0f
            import torch
            import torch.nn.functional as F
            v = [F.interpolate(masks[k][range(T), int(best[k])][None], size=size, mode="bilinear", align_corners=False)[0] for k in (0, 1)]
            ties = int(((v[0] >= _davis.V_SAT) & (v[1] >= _davis.V_SAT)).sum())
        print(f"{name}: n={n} labels {tuple(labels.shape)} best {best.tolist()} contested share {float(contested.float().mean()):.3e}"
              f" label histogram {np.bincount(labels.numpy().ravel(), minlength=n + 1).tolist()}" + (f" saturated ties {ties}" if ties else ""))
    path = os.path.join(HERE, "davis_label_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
