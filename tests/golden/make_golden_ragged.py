"""Generates tests/golden/text_pos_ragged.npz by running the REFERENCE's own PositionEmbeddingSine1D (CPU, build machine only).

Run from the repository root:  python tests/golden/make_golden_ragged.py
Needs the reference tree (ref_harness.REF_ROOT) -- never runs on the GPU box.  The file it writes is data:

  text_pos_ragged.npz  PositionEmbeddingSine1D(256, normalize=True) (models/position_encoding.py:28-50) on a [3, Lmax] key
                       padding mask of right-padded captions (what forward_text builds with padding="longest",
                       tce_rvos.py:252-300), pad positions included:
                         lens [3] int32, mask [3, Lmax] bool (True = pad), pos [3, Lmax, 256] float32 (caption, token, channel)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

LENS = (9, 4, 17)


def main():
    rh.import_reference()
    from models.position_encoding import PositionEmbeddingSine1D
    from util.misc import NestedTensor
    Lmax = max(LENS)
    mask = torch.arange(Lmax)[None, :] >= torch.tensor(LENS)[:, None]  # [3, Lmax], True = pad
    feats = torch.zeros(len(LENS), 256, Lmax)
    pos = PositionEmbeddingSine1D(256, normalize=True)(NestedTensor(feats, mask))  # [B, C, T]
    out = os.path.join(HERE, "text_pos_ragged.npz")
    np.savez_compressed(out, lens=np.array(LENS, dtype=np.int32), mask=mask.numpy(),
                        pos=pos.permute(0, 2, 1).contiguous().numpy().astype(np.float32))
    print("wrote", out, tuple(pos.shape))


if __name__ == "__main__":
    main()
