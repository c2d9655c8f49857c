"""Forward + backward of SetCriterion(grad=True) (libtce_rvos_train.so, entries (a)-(d)) against the loop a caller can write today:
fp32 autograd of the reference's formulas as torch operations on the same device tensors (tests/_criterion.py torch_form, its
.item() included), sum(w_k * loss_k).backward() on both sides with the reference's weights.

    python tools/criterion_grad_bench.py [--rounds 3]

Interleaved rounds in one process, no graph: per configuration and round, N calls of each side between two device events after a
warm-up of every shape, the host waiting for the second event.  Mask shapes of config 2 (T=5, Q=5, 360x640 -> 96x160) and config 5
(T=10, Q=5, 480x854 -> 120x216), B = 1 and 8, one decoder layer.  Entry (c) alone (ops.criterion_mask_grad into a preallocated
gradient, one launch) is timed the same way; its bytes are the whole gradient written, 4*B*T*Q*h*w, plus the matched planes
(4*B*T*h*w) and a target byte per sample (B*T*h*w) read, over the measured HBM rate of 6.29 TB/s.  That rate is bytes over the time
of back-to-back calls between events, not a kernel time from a trace.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import _criterion as R  # noqa: E402
import _criterion_grad as G  # noqa: E402
from criterion_bench import CONFIGS, make, timed  # noqa: E402
from tce_rvos_amd import ops  # noqa: E402
from tce_rvos_amd.criterion import SetCriterion  # noqa: E402

HBM_MEASURED = 6.29e12
KEYS = ("pred_logits", "pred_boxes", "pred_masks")


def weighted(losses):
    return sum(G.WEIGHTS["_".join(k.split("_")[:2])] * v for k, v in losses.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--torch-calls", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU; there is no fallback"
    crit = SetCriterion(1, {}, ["labels", "boxes", "masks"], grad=True)
    plain = SetCriterion(1, {}, ["labels", "boxes", "masks"])
    rows = []
    for name, T, Q, H, W in CONFIGS:
        for B in (1, 8):
            out, tg = make(B, T, Q, H, W, 7)
            for k in KEYS:
                out[k].requires_grad_(True)
            h, w = out["pred_masks"].shape[-2:]
            nbytes = 4 * B * T * Q * h * w + 4 * B * T * h * w + B * T * h * w

            def hip(out=out, tg=tg):
                for k in KEYS:
                    out[k].grad = None
                weighted(crit(out, tg)).backward()

            def tor(out=out, tg=tg):
                for k in KEYS:
                    out[k].grad = None
                weighted(R.torch_form(out, tg)[0]).backward()

            # the two sides agree before they are timed
            hip()
            mine = {k: out[k].grad.clone() for k in KEYS}
            tor()
            for k in KEYS:
                d, top = float((mine[k] - out[k].grad).abs().max()), float(out[k].grad.abs().max())
                assert d <= 1e-4 * top, (name, B, k, d, top)
            det = {k: out[k].detach() for k in KEYS}
            vals = plain.layer_values(det, tg)[0]
            tmask = torch.stack([t["masks"] for t in tg])
            num_boxes = plain._num_boxes(tg, tmask.device)
            gl = torch.tensor(G.gl_of(), dtype=torch.float32, device="cuda")
            grad = torch.empty_like(det["pred_masks"])

            def entry_c(det=det, tmask=tmask, vals=vals, num_boxes=num_boxes, gl=gl, grad=grad):
                ops.criterion_mask_grad(det["pred_masks"], tmask, vals["sums"], vals["st"], vals["index"], num_boxes, gl, out=grad)

            sides = {"hip": hip, "torch": tor, "c": entry_c}
            for fn in sides.values():  # warm-up of every shape
                for _ in range(3):
                    fn()
            rows.append((name, B, nbytes, sides, {"hip": [], "torch": [], "c": []}))
    for r in range(a.rounds):
        for name, B, nbytes, sides, t in rows:
            t["hip"].append(timed(sides["hip"], a.calls))
            t["torch"].append(timed(sides["torch"], a.torch_calls))
            t["c"].append(timed(sides["c"], a.calls))
    print(f"device {torch.cuda.get_device_name(0)}; us per call, {a.rounds} interleaved rounds (each: {a.calls} HIP calls, {a.torch_calls} "
          f"torch calls); measured HBM rate {HBM_MEASURED / 1e12:.2f} TB/s")
    for name, B, nbytes, sides, t in rows:
        hip, tor, c = (sorted(t[k])[len(t[k]) // 2] for k in ("hip", "torch", "c"))
        print(f"{name} B={B}: forward+backward HIP {hip:8.1f} us (rounds {', '.join('%.1f' % v for v in t['hip'])})   torch autograd "
              f"{tor:9.1f} us (rounds {', '.join('%.1f' % v for v in t['torch'])})   ratio {tor / hip:6.1f}x   entry (c) {c:7.1f} us, "
              f"{nbytes / 1e6:.2f} MB -> {nbytes / (c * 1e-6) / 1e9:7.1f} GB/s = {100 * nbytes / (c * 1e-6) / HBM_MEASURED:5.2f}% of the "
              f"measured HBM rate (rounds {', '.join('%.1f' % v for v in t['c'])})", flush=True)


if __name__ == "__main__":
    main()
