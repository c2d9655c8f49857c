"""Ref-DAVIS J&F restated in NumPy alone: db_eval_iou (davis2017/metrics.py:6-37), _seg2bmap (:122-178 at equal size) and f_measure
(:57-119) of the reference, with its two libraries replaced by what they compute: skimage's disk(r) is the offsets with
dx*dx + dy*dy <= r*r, and cv2.dilate with that kernel (default border: nothing beyond the plane) is the OR of the plane's copies
shifted by those offsets.  np.bool (removed from NumPy) becomes bool.  Nothing here touches the library under test.

Also the case table of the scoring tests and the makers of their label maps.  Used by tests/golden/make_golden_jf.py, which
writes jf_cases.npz from it, and by the tests, which run it for the shape too large to commit."""
import numpy as np

# ------------------------------------------------------------------------------------------------------------ the reference


def db_eval_iou(annotation, segmentation):
    """metrics.py:16-37 for one frame (void_pixels=None) -> (inters, union, j)"""
    assert annotation.shape == segmentation.shape
    annotation = annotation.astype(bool)
    segmentation = segmentation.astype(bool)
    void_pixels = np.zeros_like(segmentation)
    inters = np.sum((segmentation & annotation) & np.logical_not(void_pixels), axis=(-2, -1))
    union = np.sum((segmentation | annotation) & np.logical_not(void_pixels), axis=(-2, -1))
    with np.errstate(divide="ignore", invalid="ignore"):
        j = inters / union
    if j.ndim == 0:
        j = 1 if np.isclose(union, 0) else j
    else:
        j[np.isclose(union, 0)] = 1
    return int(inters), int(union), float(j)


def seg2bmap(seg):
    """metrics.py:137-168 with width = w, height = h"""
    seg = seg.astype(bool)
    seg[seg > 0] = 1
    assert np.atleast_3d(seg).shape[2] == 1
    e = np.zeros_like(seg)
    s = np.zeros_like(seg)
    se = np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = seg ^ e | seg ^ s | seg ^ se
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = 0
    return b


def disk(radius):
    """skimage.morphology.disk: uint8 [2r+1, 2r+1], 1 where dx*dx + dy*dy <= r*r"""
    r = int(radius)
    L = np.arange(-r, r + 1)
    X, Y = np.meshgrid(L, L)
    return np.array((X ** 2 + Y ** 2) <= r ** 2, dtype=np.uint8)


def dilate(b, radius):
    """cv2.dilate(b, disk(radius)): the OR of the copies of b shifted by the disk's offsets, nothing entering from beyond the plane"""
    b = b.astype(bool)
    H, W = b.shape
    r = int(radius)
    out = np.zeros_like(b)
    d = disk(r)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if not d[dy + r, dx + r]:
                continue
            # out[y, x] |= b[y + dy, x + dx]
            ys0, ys1 = max(0, dy), min(H, H + dy)
            xs0, xs1 = max(0, dx), min(W, W + dx)
            if ys0 >= ys1 or xs0 >= xs1:
                continue
            out[ys0 - dy:ys1 - dy, xs0 - dx:xs1 - dx] |= b[ys0:ys1, xs0:xs1]
    return out.astype(np.uint8)


def f_measure(foreground_mask, gt_mask, bound_pix):
    """metrics.py:80-119 with void_pixels=None and the radius given -> (n_fg, n_gt, sum(fg_match), sum(gt_match), F)"""
    void_pixels = np.zeros_like(foreground_mask).astype(bool)
    fg_boundary = seg2bmap(foreground_mask * np.logical_not(void_pixels))
    gt_boundary = seg2bmap(gt_mask * np.logical_not(void_pixels))
    fg_dil = dilate(fg_boundary.astype(np.uint8), bound_pix)
    gt_dil = dilate(gt_boundary.astype(np.uint8), bound_pix)
    gt_match = gt_boundary * fg_dil
    fg_match = fg_boundary * gt_dil
    n_fg = np.sum(fg_boundary)
    n_gt = np.sum(gt_boundary)
    if n_fg == 0 and n_gt > 0:
        precision = 1
        recall = 0
    elif n_fg > 0 and n_gt == 0:
        precision = 0
        recall = 1
    elif n_fg == 0 and n_gt == 0:
        precision = 1
        recall = 1
    else:
        precision = np.sum(fg_match) / float(n_fg)
        recall = np.sum(gt_match) / float(n_gt)
    if precision + recall == 0:
        F = 0
    else:
        F = 2 * precision * recall / (precision + recall)
    return int(n_fg), int(n_gt), int(np.sum(fg_match)), int(np.sum(gt_match)), float(F)


def reference(pred, gt, n, radius):
    """pred, gt uint8 [T,H,W] label maps -> (counts int64 [n,T,6], J float64 [n,T], F float64 [n,T]): per object k, seg = (pred == k+1)
    and ann = (gt == k+1), as davis.py:95-98 and results.py separate the objects of a label map"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    T = pred.shape[0]
    counts = np.zeros((n, T, 6), dtype=np.int64)
    J, F = np.zeros((n, T)), np.zeros((n, T))
    for k in range(n):
        for t in range(T):
            seg, ann = pred[t] == k + 1, gt[t] == k + 1
            i, u, J[k, t] = db_eval_iou(ann, seg)
            n_fg, n_gt, fm, gm, F[k, t] = f_measure(seg, ann, radius)
            counts[k, t] = (i, u, n_fg, n_gt, fm, gm)
    return counts, J, F


# --------------------------------------------------------------------------------------------------------------- the cases
# name, seed, T, n, H, W, radius, kind
CASES = (("A", 71, 3, 2, 7, 9, 1, "blobs"),        # smaller than any tile or word
         ("B", 72, 2, 3, 33, 65, 2, "blobs"),      # one past a 64-bit word; odd W: unaligned rows
         ("C", 73, 2, 2, 70, 131, 3, "borders"),   # objects on all four borders and in the bottom-right corner, 255 in gt, n+1 in pred
         ("D", 74, 1, 1, 40, 200, 5, "pixels"),    # single pixels whose boundary blocks sit at and just beyond the disk's rim
         ("E", 75, 4, 2, 20, 70, 2, "empties"),    # pred empty / gt empty / both empty / identical
         ("F", 76, 2, 16, 48, 300, 18, "blobs"),   # the 1080p radius and the object limit
         ("G", 77, 2, 3, 150, 300, 8, "sparse"))   # sparse blobs over many tiles
FULL = ("full", 78, 2, 3, 480, 854, 8, "sparse")   # computed in the test, not committed

# case D: (dy, dx) of the ann pixel from the seg pixel.  A single pixel's boundary is the 2x2 block up and left of it, so the
# NEAREST pair of boundary pixels of the two blocks lies one step closer in every non-zero component: (5,0), (3,4), (0,-5) -- on the
# rim of disk(5), must match -- and (4,4), (5,1), (6,0) -- just beyond it, must not.
D_MATCH = ((6, 0), (4, 5), (0, -6))
D_MISS = ((5, 5), (6, 2), (7, 0))
# (y, first x, offset): repeated at x + 61*j, j = 0..2, so pairs straddle columns 64 and 128 and rows 31/32
D_SLOTS = ((4, 8, (0, -6)), (4, 28, (6, 0)), (4, 48, (7, 0)), (27, 18, (5, 5)), (27, 38, (6, 2)), (27, 59, (4, 5)))


def _discs(rng, H, W, n, per_obj, rmax):
    """label map [H,W]: per object `per_obj` discs of random centre and radius, later objects over earlier ones"""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), dtype=np.uint8)
    spec = []
    for k in range(n):
        for _ in range(per_obj):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.uniform(1.0, rmax)
            spec.append((k + 1, cy, cx, r))
            m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k + 1
    return m, spec


def _jitter(rng, H, W, spec, shift, grow):
    """the same discs moved by up to `shift` pixels and grown by up to +-`grow`: a prediction near its ground truth"""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), dtype=np.uint8)
    for lab, cy, cx, r in spec:
        cy, cx = cy + rng.integers(-shift, shift + 1), cx + rng.integers(-shift, shift + 1)
        r = max(0.5, r + rng.uniform(-grow, grow))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = lab
    return m


def make_case(case):
    """(pred, gt) uint8 [T,H,W] of a row of CASES / FULL"""
    name, seed, T, n, H, W, radius, kind = case
    rng = np.random.default_rng(seed)
    pred, gt = np.zeros((T, H, W), dtype=np.uint8), np.zeros((T, H, W), dtype=np.uint8)
    if kind in ("blobs", "sparse"):
        per_obj, rmax = (2, max(2.0, min(H, W) / 4)) if kind == "blobs" else (3, min(H, W) / 8)
        for t in range(T):
            gt[t], spec = _discs(rng, H, W, n, per_obj, rmax)
            pred[t] = _jitter(rng, H, W, spec, max(1, radius), max(1.0, radius / 2))
    elif kind == "borders":
        for t in range(T):
            g = gt[t]
            g[0:6, 20:60] = 1            # top border
            g[H - 5:H, 10:50] = 2        # bottom border
            g[20:50, 0:4] = 1            # left border
            g[10:40, W - 3:W] = 2        # right border
            g[H - 7:H, W - 9:W] = 1      # bottom-right corner
            g[0:3, 0:3] = 2              # top-left corner
            g[H - 1, 60:70] = 1          # a run in the last row alone
            g[30:36, 64 - 2:64 + 3] = 2  # across the word seam
            g[30:34, 70:80] = 255        # void: belongs to no object
            p = pred[t]
            p[0:5, 22:63] = 1
            p[H - 6:H, 12:49] = 2
            p[22:52, 0:5] = 1
            p[8:41, W - 2:W] = 2
            p[H - 6:H, W - 8:W] = 1
            p[0:2, 0:4] = 2
            p[H - 1, 58:66] = 1
            p[31:37, 64 - 3:64 + 2] = 2
            p[40:50, 90:100] = n + 1     # a label above n: belongs to no object
            p[H - 2:H, W - 2:W] = 2 if t else 1
    elif kind == "pixels":
        assert radius == 5 and n == 1
        for y, x, (dy, dx) in D_SLOTS:
            for j in range(3):
                pred[0, y, x + 61 * j] = 1
                gt[0, y + dy, x + 61 * j + dx] = 1
    elif kind == "empties":
        g, spec = _discs(rng, H, W, n, 2, 6.0)
        p = _jitter(rng, H, W, spec, 2, 1.0)
        gt[0], pred[0] = g, 0            # the prediction is empty
        gt[1], pred[1] = 0, p            # the ground truth is empty
        gt[2], pred[2] = 0, 0            # both are empty
        gt[3], pred[3] = g, g            # identical
    else:
        raise ValueError(kind)
    return pred, gt


def load_cases(path):
    """The committed fixture -> {name: dict(pred, gt, n, radius, counts, J, F)}"""
    fx = np.load(path)
    out = {}
    for name in [str(s) for s in fx["names"]]:
        out[name] = {"pred": fx[f"{name}_pred"], "gt": fx[f"{name}_gt"], "n": int(fx[f"{name}_n"]), "radius": int(fx[f"{name}_radius"]),
                     "counts": fx[f"{name}_counts"], "J": fx[f"{name}_J"], "F": fx[f"{name}_F"]}
    return out
