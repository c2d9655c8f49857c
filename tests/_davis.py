"""The Ref-DAVIS caller stage restated with the PyTorch primitives the reference's driver uses (inference_davis.py:239-248 per
object, :293-298 per annotator), the acceptance rule of the label-map tests, and the fixture's case table.

Used by tests/golden/make_golden_davis.py (which writes davis_label_cases.npz from it) and by the tests, which run it on the CPU
for shapes too large to commit.  Pure torch on whatever device the inputs are on; nothing here touches the library under test.

Acceptance rule.  A pixel is CONTESTED when the reference's own label hangs on rounding:
  (i)  some object has |v_k| <= V_EPS (v_k = its up-sampled mask logit): sigmoid(v_k) is within rounding of the 0.5 threshold;
  (ii) the two largest of [background, s_1 .. s_n] differ by <= S_EPS -- unless both are objects with v >= V_SAT, whose scores are
       exactly 1.0f in any fp32 sigmoid (exp(-20) < 2^-24): that tie is exact, and the first maximum must win.
Labels must equal the reference on every other pixel and be <= n everywhere; the contested share of a case must stay <= MAX_SHARE,
or the rule could hide a failure.  The constants come from fp32: interpolation of |v| <= 50 rounds to a few 1e-6 at most, and a
sigmoid's last bits are below 1e-6 wherever the score passes the threshold."""
import numpy as np
import torch
import torch.nn.functional as F

V_EPS, S_EPS, V_SAT, MAX_SHARE = 1e-5, 1e-6, 20.0, 0.01

# case, seed, n, T, Q, (h, w), (H0, W0), scale
CASES = (("A", 31, 3, 4, 5, (23, 40), (90, 160), 3.0),
         ("B", 32, 5, 3, 5, (30, 54), (120, 214), 3.0),
         ("D", 34, 3, 3, 5, (23, 40), (90, 160), 3.0),   # + saturated blocks on objects 0 and 1 (make_inputs)
         ("E", 35, 3, 3, 5, (23, 40), (97, 151), 8.0))   # odd sizes


def make_inputs(name, seed, n, T, Q, hw, scale):
    """logits [n,T,Q,1] and masks [n,T,Q,h,w] of a case, from torch.Generator(seed)."""
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    logits = torch.randn(n, T, Q, 1, generator=g)
    masks = torch.randn(n, T, Q, h, w, generator=g) * scale
    if name == "D":  # two objects saturate (sigmoid = 1.0f exactly) on overlapping blocks: score ties that object 0 must win
        b = masks[0, :, :, h // 4:h // 2, w // 4:3 * w // 4]
        masks[0, :, :, h // 4:h // 2, w // 4:3 * w // 4] = 25 + b.abs()
        b = masks[1, :, :, h // 3:2 * h // 3, w // 3:2 * w // 3]
        masks[1, :, :, h // 3:2 * h // 3, w // 3:2 * w // 3] = 40 + b.abs()
    return logits, masks


def best_query(pred_logits):
    """inference_davis.py:239-243 for one object's pred_logits [t,q,k] -> python int"""
    pred_scores = pred_logits.sigmoid()      # [t, q, k]
    pred_scores = pred_scores.mean(0)        # [q, K]
    max_scores, _ = pred_scores.max(-1)      # [q,]
    _, max_ind = max_scores.max(-1)          # [1,]
    return int(max_ind)


def reference_labels(logits, masks, out_hw, threshold=0.5, background=0.1):
    """logits / masks: sequences of n tensors [T,Q,K] / [T,Q,h,w].  Returns (labels uint8 [T,H0,W0], best int32 [n], contested bool
    [T,H0,W0]) -- the driver's label map, its query choice, and the pixels where that label hangs on rounding (module docstring)."""
    n = len(logits)
    best, vs = [], []
    for pred_logits, pred_masks in zip(logits, masks):
        clip_len = pred_logits.shape[0]
        max_ind = best_query(pred_logits)
        max_inds = torch.tensor([max_ind]).repeat(clip_len)
        pm = pred_masks[range(clip_len), max_inds, ...]  # [t, h, w]
        pm = pm.unsqueeze(0)
        pm = F.interpolate(pm, size=tuple(out_hw), mode="bilinear", align_corners=False)
        best.append(max_ind)
        vs.append(pm[0])
    v = torch.stack(vs)                      # [n, t, H0, W0] up-sampled logits
    anno_masks = v.sigmoid()                 # NOTE: here mask is score
    t, h, w = anno_masks.shape[-3:]
    anno_masks[anno_masks < threshold] = 0.0
    bg = background * torch.ones(1, t, h, w, device=v.device)
    anno_masks = torch.cat([bg, anno_masks], dim=0)   # [n+1, t, H0, W0]
    out_masks = torch.argmax(anno_masks, dim=0)
    top, idx = anno_masks.topk(2, dim=0)
    vb = torch.cat([torch.full_like(v[:1], -1.0), v], 0)  # the background never counts as saturated
    sat = (idx > 0) & (vb.gather(0, idx) >= V_SAT)
    contested = (v.abs() <= V_EPS).any(0) | (((top[0] - top[1]) <= S_EPS) & ~(sat[0] & sat[1]))
    assert int(out_masks.max()) <= n
    return out_masks.to(torch.uint8), torch.tensor(best, dtype=torch.int32), contested


def check_labels(got, want, contested, n, what=""):
    """The acceptance rule; prints the figures before it asserts.  got / want uint8 [T,H0,W0], contested bool (all on the CPU)."""
    got, want, contested = got.cpu(), want.cpu(), contested.cpu()
    share = float(contested.float().mean())
    bad = (got != want) & ~contested
    print(f"{what}: {got.numel()} pixels, contested share {share:.3e}, mismatches outside contested {int(bad.sum())}, "
          f"inside {int(((got != want) & contested).sum())}, max label {int(got.max())}")
    assert share <= MAX_SHARE, f"{what}: contested share {share:.3e} above {MAX_SHARE}: the rule would hide a failure"
    assert int(got.max()) <= n, f"{what}: label {int(got.max())} with {n} objects"
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} labels differ from the reference outside contested pixels"
    return share


def load_cases(path):
    """The committed fixture -> list of dicts(name, n, logits, masks, size, best, labels, contested) of CPU tensors."""
    fx = np.load(path)
    out = []
    for name in [str(s) for s in fx["names"]]:
        labels = torch.from_numpy(fx[f"{name}_labels"])
        c = np.unpackbits(fx[f"{name}_contested"])[:labels.numel()].reshape(tuple(labels.shape)).astype(bool)
        masks = np.ascontiguousarray(fx[f"{name}_masks_bytes"].T).view(np.float32).reshape(tuple(fx[f"{name}_masks_shape"]))
        out.append({"name": name, "logits": torch.from_numpy(fx[f"{name}_logits"]), "masks": torch.from_numpy(masks),
                    "size": tuple(int(s) for s in fx[f"{name}_size"]), "best": torch.from_numpy(fx[f"{name}_best"]),
                    "labels": labels, "contested": torch.from_numpy(c), "n": int(fx[f"{name}_logits"].shape[0])})
    return out
