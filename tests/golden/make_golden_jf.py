"""Writes tests/golden/jf_cases.npz: the label maps of tests/_jf.py's cases A-G and what the NumPy restatement of the reference's
davis2017/metrics.py (tests/_jf.py) makes of them -- the six counts, J and F per (object, frame).  Runs anywhere NumPy runs:

    python tests/golden/make_golden_jf.py

Where SciPy imports, the shifted-copy dilation of the restatement is first held to scipy.ndimage.binary_dilation with the disk as
structure, on every boundary map of every case."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _jf  # noqa: E402

try:
    from scipy.ndimage import binary_dilation
except ImportError:
    binary_dilation = None

out = {"names": np.array([c[0] for c in _jf.CASES])}
for case in _jf.CASES:
    name, seed, T, n, H, W, radius, kind = case
    pred, gt = _jf.make_case(case)
    if binary_dilation is not None:
        for k in range(n):
            for t in range(T):
                for m in (pred[t] == k + 1, gt[t] == k + 1):
                    b = _jf.seg2bmap(m)
                    assert np.array_equal(_jf.dilate(b, radius).astype(bool), binary_dilation(b, structure=_jf.disk(radius).astype(bool))), (name, k, t)
    counts, J, F = _jf.reference(pred, gt, n, radius)
    if name == "D":  # the rim of the disk: pairs on it match in one pixel or more, pairs just beyond it in none
        hits = sum(1 for _, _, d in _jf.D_SLOTS if d in _jf.D_MATCH) * 3
        assert counts[0, 0, 2] == counts[0, 0, 3] == 4 * 3 * len(_jf.D_SLOTS), counts
        assert counts[0, 0, 4] == counts[0, 0, 5] == 2 * 3 + 2 * 3 + 1 * 3 and hits == 9, counts  # (6,0): 2, (0,-6): 2, (4,5): 1
    out[f"{name}_pred"], out[f"{name}_gt"] = pred, gt
    out[f"{name}_n"], out[f"{name}_radius"] = np.int32(n), np.int32(radius)
    out[f"{name}_counts"], out[f"{name}_J"], out[f"{name}_F"] = counts, J, F
    print(f"case {name}: T={T} n={n} {H}x{W} radius {radius}: counts sum {counts.sum(axis=(0, 1)).tolist()}, "
          f"J mean {J.mean():.4f}, F mean {F.mean():.4f}, scipy {'checked' if binary_dilation is not None else 'absent'}")
path = os.path.join(HERE, "jf_cases.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
