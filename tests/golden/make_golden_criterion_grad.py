"""Generates tests/golden/criterion_grad_cases.npz: the gradients of the reference's own SetCriterion (models/criterion.py, with its
HungarianMatcher) by torch autograd on the CPU, on the cases of tests/_criterion.py with inputs that require grad -- build machine
only; the reference is imported through ref_harness.

Run from the repository root:  python tests/golden/make_golden_criterion_grad.py
The file it writes is data; the inputs regenerate from the seeds of the case table.  Every loss key is backpropagated on its own
(retain_graph) and the per-key gradients are combined in fp64 with the reference's weights (_criterion_grad.WEIGHTS), which is what
sum(w_k * loss_k).backward() yields.  Per case X (c1 .. c10) and layer L (0 = the last decoder layer, 1.. = aux layer L-1):
  X_g_logits<L> [B,T,Q,K], X_g_boxes<L> [B,T,Q,4], X_g_visible<L> [B,T,Q,1] f32   the weighted gradients
  X_g_masks<L> [B,T,h,w] f32      the matched query's planes of pred_masks' gradient; the other planes are asserted exactly zero
  X_margin_<tensor><L> f32        the reference's distance from the fp64 closed form (_criterion_grad.grad_layer), rounded upwards

Conditions asserted here, so that the reference alone stays inside them: the match equals the restatement's; every pair of corner
coordinates that a min / max compares, every |p_j - g_j| and every non-clamped extent of a matched box exceeds 1e-4 (torch splits or
picks a sub-gradient at those kinks); each loss key reaches only the tensors it is a function of; the recorded margin stays within
the derived bound plus the reference's allowance (_criterion_grad's docstring: its fp32 sums through R.ref_sum_bound, its
subtractions, its own reverse chain).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _criterion as R  # noqa: E402
import _criterion_grad as G  # noqa: E402
import ref_harness  # noqa: E402

TOUCHES = {"loss_ce": {"pred_logits"}, "loss_bbox": {"pred_boxes"}, "loss_giou": {"pred_boxes"}, "loss_mask": {"pred_masks"},
           "loss_dice": {"pred_masks"}, "loss_vis": {"pred_visible"}}


def _leaves(o):
    return {k: v.clone().requires_grad_(True) for k, v in o.items() if k != "aux_outputs"}


def main():
    args = ref_harness.reference_args()
    ref_harness.build_reference_model(args, roberta_layers=1)  # puts the reference on the path with the stand-ins it needs
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    out = {}
    c = R.CONSTS
    for case in R.CASES:
        name, seed, B, T, Q, K, (H, W), valid, vis, n_aux = case
        outputs, targets = R.make_case(case)
        matcher = HungarianMatcher(cost_class=c["cost_class"], cost_bbox=c["cost_bbox"], cost_giou=c["cost_giou"],
                                   cost_mask=c["cost_mask"], cost_dice=c["cost_dice"], cost_vis=c["cost_vis"], num_classes=K,
                                   masks=True, vis=vis)
        losses = ["labels", "boxes", "masks"] + (["visible"] if vis else [])
        crit = SetCriterion(K, matcher=matcher, weight_dict={}, eos_coef=0.1, losses=losses, focal_alpha=c["focal_alpha"])
        leaves = _leaves(outputs)
        if n_aux:
            leaves["aux_outputs"] = [_leaves(a) for a in outputs["aux_outputs"]]
        layer_leaves = [leaves] + list(leaves.get("aux_outputs", []))
        ref_losses = crit(leaves, targets)
        with torch.no_grad():
            indices = [matcher(o, targets) for o in [outputs] + list(outputs.get("aux_outputs", []))]
        mine, restated, num_boxes = G.grads(outputs, targets, vis=vis)
        total = [{k: torch.zeros_like(v, dtype=torch.float64) for k, v in lv.items() if k != "aux_outputs"} for lv in layer_leaves]
        for key, value in ref_losses.items():
            parts = key.split("_")
            base, L = "_".join(parts[:2]), (int(parts[2]) + 1 if len(parts) == 3 else 0)
            flat = [(l, k, v) for l, lv in enumerate(layer_leaves) for k, v in lv.items() if k != "aux_outputs"]
            got = torch.autograd.grad(value, [v for _, _, v in flat], retain_graph=True, allow_unused=True)
            for (l, k, _), g in zip(flat, got):
                reached = g is not None and bool((g != 0).any())
                assert not reached or (l == L and k in TOUCHES[base]), (name, key, l, k)
                if reached:
                    total[l][k] += G.WEIGHTS[base] * g.double()
        for L, (tot, g, r) in enumerate(zip(total, mine, restated)):
            index = torch.stack([i[0][0] for i in indices[L]])
            assert torch.equal(index, r["index"]), (name, L, index, r["index"])
            assert g["min_kink"] > G.KINK, (name, L, g["min_kink"])
            for short, key in G.GRAD_KEYS:
                if key not in tot:
                    continue
                ref = tot[key]
                if short == "masks":
                    assert not bool((ref[G.off_query_mask(ref.shape, index)] != 0).any()), (name, L, "off-query planes")
                    ref = G.matched_planes(ref, index)
                ref32 = ref.float()
                margin = (ref32.double() - g["g_" + short]).abs()
                allowed = g["e_" + short] + g["a_" + short]
                worst = float((margin - allowed).max())
                print(f"{name} layer {L} {short}: max |g| {float(ref.abs().max()):.3e} reference-closed form {float(margin.max()):.3e} "
                      f"bound max {float(g['e_' + short].max()):.3e} allowance max {float(g['a_' + short].max()):.3e} kink "
                      f"{g['min_kink']:.2e}")
                assert worst <= 0, (name, L, short, worst)
                m32 = margin.numpy().astype(np.float32)
                m32 = np.where(m32.astype(np.float64) < margin.numpy(), np.nextafter(m32, np.float32(np.inf)), m32)
                out[f"{name}_g_{short}{L}"], out[f"{name}_margin_{short}{L}"] = ref32.numpy(), m32
    path = os.path.join(HERE, "criterion_grad_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 2_000_000


if __name__ == "__main__":
    main()
