"""SetCriterion on the GPU (libtce_rvos_train.so) against the loop a caller writes today: the reference's formulas as torch
operations on the same device tensors (tests/_criterion.py torch_form, its .item() and its per-frame `if valid` included).

    python tools/criterion_bench.py [--rounds 3]

Three interleaved rounds in one process, no graph: per configuration and round, N calls of each side between two device events
after a warm-up, the host waiting for the second event (the torch loop synchronises by itself; the HIP path never does, so its
figure is the device time of back-to-back calls).  Mask shapes of config 2 (T=5, Q=5, 360x640 -> 96x160) and config 5 (T=10, Q=5,
480x854 -> 120x216), B = 1 and 8, one decoder layer.  Launch (a) alone (tce_criterion_mask_sums_f64, both of its kernels) is timed
the same way; its bytes are the fp32 mask logits read once plus one target byte per element, over the 8 TB/s HBM peak.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import _criterion as R  # noqa: E402
from tce_rvos_amd import ops  # noqa: E402
from tce_rvos_amd.criterion import SetCriterion  # noqa: E402

HBM_PEAK = 8.0e12
CONFIGS = [("cfg2", 5, 5, 360, 640), ("cfg5", 10, 5, 480, 854)]


def make(B, T, Q, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    h, w = R.ceil32(H) // 4, R.ceil32(W) // 4
    out = {k: v.cuda() for k, v in R._layer_inputs(g, B, T, Q, 1, h, w, False).items()}
    targets = []
    for b in range(B):
        boxes = torch.cat([0.3 + 0.4 * torch.rand(T, 2, generator=g), 0.15 + 0.35 * torch.rand(T, 2, generator=g)], -1)
        masks = torch.zeros(T, H, W, dtype=torch.uint8)
        masks[:, H // 4:H // 2, W // 3:2 * W // 3] = 1
        targets.append({"masks": masks.cuda(), "boxes": boxes.cuda(), "labels": torch.zeros(T, dtype=torch.int64).cuda(),
                        "valid": torch.ones(T, dtype=torch.int64).cuda()})
    return out, targets


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--torch-calls", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU; there is no fallback"
    crit = SetCriterion(1, {}, ["labels", "boxes", "masks"])
    rows = []
    for name, T, Q, H, W in CONFIGS:
        for B in (1, 8):
            out, tg = make(B, T, Q, H, W, 7)
            tmask = torch.stack([t["masks"] for t in tg])
            h, w = out["pred_masks"].shape[-2:]
            nbytes = B * T * Q * h * w * 4 + B * T * h * w  # what launch (a) must read: the logits once, a target byte per sample
            sides = {"hip": lambda out=out, tg=tg: crit(out, tg), "torch": lambda out=out, tg=tg: R.torch_form(out, tg),
                     "sums": lambda out=out, tmask=tmask: ops.criterion_mask_sums(out["pred_masks"], tmask)}
            # the two sides agree before they are timed
            mine, theirs = crit(out, tg), R.torch_form(out, tg)[0]
            for k in mine:
                assert abs(float(mine[k]) - float(theirs[k])) <= 1e-4 * max(1.0, abs(float(theirs[k]))), (k, float(mine[k]), float(theirs[k]))
            for k, fn in sides.items():  # warm-up of every shape
                for _ in range(3):
                    fn()
            rows.append((name, B, nbytes, sides, {"hip": [], "torch": [], "sums": []}))
    for r in range(a.rounds):
        for name, B, nbytes, sides, t in rows:
            t["hip"].append(timed(sides["hip"], a.calls))
            t["torch"].append(timed(sides["torch"], a.torch_calls))
            t["sums"].append(timed(sides["sums"], a.calls))
    print(f"device {torch.cuda.get_device_name(0)}; us per call, {a.rounds} interleaved rounds (each: {a.calls} HIP calls, {a.torch_calls} torch "
          f"calls); HBM peak {HBM_PEAK / 1e12:.1f} TB/s")
    for name, B, nbytes, sides, t in rows:
        hip, tor, sums = (sorted(t[k])[len(t[k]) // 2] for k in ("hip", "torch", "sums"))
        print(f"{name} B={B}: criterion HIP {hip:8.1f} us (rounds {', '.join('%.1f' % v for v in t['hip'])})   torch loop {tor:9.1f} us "
              f"(rounds {', '.join('%.1f' % v for v in t['torch'])})   ratio {tor / hip:6.1f}x   launch (a) {sums:7.1f} us, "
              f"{nbytes / 1e6:.2f} MB -> {nbytes / (sums * 1e-6) / 1e9:7.1f} GB/s = {100 * nbytes / (sums * 1e-6) / HBM_PEAK:5.2f}% of peak "
              f"(rounds {', '.join('%.1f' % v for v in t['sums'])})", flush=True)


if __name__ == "__main__":
    main()
