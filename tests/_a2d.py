"""The A2D-Sentences / JHMDB-Sentences post-processor restated with the PyTorch primitives the reference class uses
(models/postprocessors.py:39-47), the COCO run-length format restated as plain loops (cocoapi maskApi.c: rleEncode, rleToString,
rleFrString), the acceptance rule of the mask tests, and the fixture's case table.

Used by tests/golden/make_golden_a2d.py (which writes a2d_post_cases.npz with the reference class itself) and by the tests, which
run it on the CPU for shapes too large to commit.  Pure torch / numpy; nothing here touches the library under test.

Acceptance rule.  A pixel is CONTESTED when the reference's own bit hangs on rounding: |v - logit(threshold)| <= V_EPS, v = its
up-sampled mask logit (at threshold 0.5: |v| <= 1e-5, the V_EPS of tests/_davis.py).  The bilinear weights of a x4 up-sampling are
exact eighths, so with |v| <= 50 the interpolation rounds to a few 1e-6 at most whatever the order of its operations, and the
sigmoid is monotone.  Masks must equal the reference on every other pixel; the contested share of a case must stay <= MAX_SHARE, or
the rule could hide a failure."""
import math

import numpy as np
import torch
import torch.nn.functional as F

V_EPS, MAX_SHARE = 1e-5, 1e-3

# case, seed, N, (h, w), size, orig, kind, scale
CASES = (("A", 41, 5, (18, 25), (72, 100), (111, 150), "smooth", 6.0),   # up-sampling; rows where the float nearest index counts
         ("B", 42, 5, (23, 40), (90, 157), (87, 145), "noise", 3.0),     # crop of the padding; down-sampling; many runs
         ("C", 43, 3, (18, 25), (72, 100), (222, 239), "smooth", 6.0),   # odd W0
         ("D", 44, 2, (3, 4), (9, 13), (5, 7), "noise", 1.0))            # tiny extents


def make_inputs(seed, N, hw, kind, scale):
    """logits [N] and masks [N,h,w] of a case, from torch.Generator(seed).  smooth: a 4x5 random grid up-sampled to the plane."""
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    logits = torch.randn(N, generator=g)
    if kind == "smooth":
        masks = F.interpolate(torch.randn(N, 1, 4, 5, generator=g), size=(h, w), mode="bicubic", align_corners=True)[:, 0] * scale
    else:
        masks = torch.randn(N, h, w, generator=g) * scale
    return logits, masks.contiguous()


def logit(threshold):
    return math.log(threshold / (1.0 - threshold))


def reference_post(masks, size, orig, threshold=0.5):
    """masks [N,h,w] fp32 -> (uint8 [N,H0,W0], v fp32 [N,H0,W0]): the literal operations of postprocessors.py:39-47 for one sample
    (the reference hard-codes threshold 0.5 at :40), and the up-sampled logit v taken through the same crop and nearest resize."""
    out_masks = masks[None]                                            # [B=1, N, out_h, out_w]
    out_h, out_w = out_masks.shape[-2:]
    up = F.interpolate(out_masks, size=(out_h * 4, out_w * 4), mode="bilinear", align_corners=False)
    pred_masks = (up.sigmoid() > threshold)
    f_mask_h, f_mask_w = int(size[0]), int(size[1])
    f_pred_masks_no_pad = pred_masks[0][:, :f_mask_h, :f_mask_w].unsqueeze(1)
    processed = F.interpolate(f_pred_masks_no_pad.float(), size=(int(orig[0]), int(orig[1])), mode="nearest")
    v = F.interpolate(up[0][:, :f_mask_h, :f_mask_w].unsqueeze(1), size=(int(orig[0]), int(orig[1])), mode="nearest")
    return processed[:, 0].to(torch.uint8), v[:, 0]


def contested(v, threshold=0.5):
    return (v - logit(threshold)).abs() <= V_EPS


def check_masks(got, want, cont, what=""):
    """The acceptance rule; prints the figures before it asserts.  got / want uint8 [N,H0,W0], cont bool."""
    got, want, cont = got.cpu(), want.cpu(), cont.cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape), (got.dtype, tuple(got.shape), tuple(want.shape))
    share = float(cont.float().mean())
    bad = (got != want) & ~cont
    print(f"{what}: {got.numel()} pixels, contested share {share:.3e}, mismatches outside contested {int(bad.sum())}, "
          f"inside {int(((got != want) & cont).sum())}, ones {int((got == 1).sum())}")
    assert share <= MAX_SHARE, f"{what}: contested share {share:.3e} above {MAX_SHARE}: the rule would hide a failure"
    assert int(got.max()) <= 1, f"{what}: mask value {int(got.max())}"
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} pixels differ from the reference outside contested pixels"
    return share


# ------------------------------------------------------------------------------------------------ the COCO run-length format
def rle_counts(mask):
    """cocoapi rleEncode for one mask [H,W] (anything array-like of 0/1): the run lengths of the column-major walk, zeros first."""
    flat = np.asarray(mask).T.reshape(-1).tolist()
    counts, p, c = [], 0, 0
    for b in flat:
        if b != p:
            counts.append(c)
            c = 0
            p = b
        c += 1
    counts.append(c)
    return counts


def rle_string(counts):
    """cocoapi rleToString: counts -> bytes (differences from the count two back, 5-bit groups low first, bit 5 = more)."""
    s = bytearray()
    counts = [int(c) for c in counts]
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            s.append(c + 48)
    return bytes(s)


def rle_from_string(s):
    """cocoapi rleFrString: bytes -> counts."""
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_decode(counts, H, W):
    """counts -> uint8 mask [H,W] (cocoapi rleDecode)."""
    counts = np.asarray(counts, dtype=np.int64)
    assert int(counts.sum()) == H * W and bool((counts[1:] > 0).all()) and int(counts[0]) >= 0, "not the run lengths of an H x W mask"
    flat = np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8)
    return np.ascontiguousarray(flat.reshape(W, H).T)


def encode(fortran_mask):
    """Stands where pycocotools.mask.encode stands at postprocessors.py:48: a Fortran-order uint8 [H,W,n] -> n dicts."""
    m = np.asarray(fortran_mask)
    assert m.ndim == 3 and m.dtype == np.uint8 and m.flags["F_CONTIGUOUS"]
    return [{"size": [int(m.shape[0]), int(m.shape[1])], "counts": rle_string(rle_counts(m[:, :, i]))} for i in range(m.shape[2])]


def load_cases(path):
    """The committed fixture -> list of dicts of CPU tensors: name, logits [N], masks [N,h,w], size, orig, scores [N], ref uint8
    [N,H0,W0], contested bool [N,H0,W0], rle (N byte strings)."""
    fx = np.load(path)
    out = []
    for name in [str(s) for s in fx["names"]]:
        orig = tuple(int(s) for s in fx[f"{name}_orig"])
        N = int(fx[f"{name}_logits"].shape[0])
        shape = (N,) + orig
        n = N * orig[0] * orig[1]
        blob, ends = fx[f"{name}_rle"].tobytes(), fx[f"{name}_rle_ends"].tolist()
        out.append({"name": name, "logits": torch.from_numpy(fx[f"{name}_logits"]), "masks": torch.from_numpy(fx[f"{name}_masks"]),
                    "size": tuple(int(s) for s in fx[f"{name}_size"]), "orig": orig,
                    "scores": torch.from_numpy(fx[f"{name}_scores"]),
                    "ref": torch.from_numpy(np.unpackbits(fx[f"{name}_ref"])[:n].reshape(shape)),
                    "contested": torch.from_numpy(np.unpackbits(fx[f"{name}_contested"])[:n].reshape(shape).astype(bool)),
                    "rle": [blob[a:b] for a, b in zip([0] + ends[:-1], ends)]})
    return out
