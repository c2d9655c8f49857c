"""Generates tests/golden/criterion_cases.npz: the reference's own HungarianMatcher (models/matcher.py) and SetCriterion
(models/criterion.py) run on the CPU on the cases of tests/_criterion.py, and the weight_dict of the reference's build()
(models/tce_rvos.py:686-715) for aux_loss on / off and vis_loss on / off -- build machine only; the reference is imported through
ref_harness.

Run from the repository root:  python tests/golden/make_golden_criterion.py
The file it writes is data; the inputs regenerate from the seeds of the case table.  Per case X (c1 .. c10) and layer L (0 = the last
decoder layer, 1.. = aux layer L-1):
  X_cost<L> [B,Q] f32, X_index<L> [B] i64     the matcher's cost column (the argument of its torch.min) and its match
  X_loss_names, X_loss_values f32             the criterion's loss dict, in its order
  X_margin_cost<L> [B,Q], X_margin_losses f64 the reference's own distance from the fp64 restatement (_criterion.restate): it sums
                                              in fp32, so a comparison against it gets this much on top of the derived bound
weight_a<aux>_v<vis>_names / _values: the weight_dict of build() for the four settings.

Conditions asserted here, so that the reference alone stays inside them: the restatement's match is the reference's; the gap between
the smallest and the second-smallest cost of a clip exceeds 10x the derived cost bound and 1e-3 of the column's spread; no box is
degenerate (every union and enclosing area exceeds MIN_AREA); the reference's distance from the restatement stays within the derived
bound plus the worst case of its fp32 sums.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _criterion as R  # noqa: E402
import ref_harness  # noqa: E402

MIN_AREA = 1e-3


def main():
    args = ref_harness.reference_args()
    ref_harness.build_reference_model(args, roberta_layers=1)  # installs the RoBERTa / tokenizer stand-ins build() needs
    import models.tce_rvos as ref_tce
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    out = {}
    for aux in (0, 1):
        for vis in (0, 1):
            a = ref_harness.reference_args(extra=([] if aux else ["--no_aux_loss"]) + (["--vis_loss"] if vis else []))
            _, crit, _ = ref_tce.build(a)
            assert isinstance(crit, SetCriterion) and crit.losses == ["labels", "boxes", "masks"] + (["visible"] if vis else [])
            out[f"weight_a{aux}_v{vis}_names"] = np.asarray(list(crit.weight_dict))
            out[f"weight_a{aux}_v{vis}_values"] = np.asarray(list(crit.weight_dict.values()), dtype=np.float64)
    c = R.CONSTS
    for case in R.CASES:
        name, seed, B, T, Q, K, (H, W), valid, vis, n_aux = case
        outputs, targets = R.make_case(case)
        matcher = HungarianMatcher(cost_class=c["cost_class"], cost_bbox=c["cost_bbox"], cost_giou=c["cost_giou"],
                                   cost_mask=c["cost_mask"], cost_dice=c["cost_dice"], cost_vis=c["cost_vis"], num_classes=K,
                                   masks=True, vis=vis)
        losses = ["labels", "boxes", "masks"] + (["visible"] if vis else [])
        crit = SetCriterion(K, matcher=matcher, weight_dict={}, eos_coef=0.1, losses=losses, focal_alpha=c["focal_alpha"])
        columns = []
        real_min = torch.min

        def recording_min(*a, **k):  # matcher.py:235: the cost column is the argument of the matcher's only torch.min
            if k.get("dim") == 0 and a[0].dim() == 2 and a[0].shape[1] == 1:
                columns.append(a[0][:, 0].clone())
            return real_min(*a, **k)

        torch.min = recording_min
        try:
            ref_losses = crit(outputs, targets)
            indices = [matcher(o, targets) for o in [outputs] + list(outputs.get("aux_outputs", []))]
        finally:
            torch.min = real_min
        n_layers = 1 + n_aux
        assert len(columns) == 2 * n_layers * B
        layers, num_boxes = R.restate(outputs, targets, c, masks=True, vis=vis)
        names = []
        for L in range(n_layers):
            cost = torch.stack(columns[L * B:(L + 1) * B])
            index = torch.stack([i[0][0] for i in indices[L]])
            r = layers[L]
            assert r["min_den"] > MIN_AREA, (name, r["min_den"])
            assert torch.equal(index, r["index"]), (name, L, index, r["index"])
            N = T * (R.ceil32(H) // 4) * (R.ceil32(W) // 4)
            margin = (cost.double() - r["cost"]).abs()
            allowed = r["e_cost"] + R.ref_sum_bound(N) * (c["cost_mask"] + c["cost_dice"]) * 2
            assert bool((margin <= allowed).all()), (name, L, margin, allowed)
            for b in range(B):
                srt = r["cost"][b].sort().values
                if Q > 1:
                    gap, spread = float(srt[1] - srt[0]), float(srt[-1] - srt[0])
                    assert gap > 10 * float(r["e_cost"][b].max()) and gap > 1e-3 * spread, (name, L, b, gap, float(r["e_cost"][b].max()))
            out[f"{name}_cost{L}"], out[f"{name}_index{L}"] = cost.numpy(), index.numpy()
            out[f"{name}_margin_cost{L}"] = margin.numpy()
            names += [k + ("" if L == 0 else f"_{L - 1}") for k in R.loss_names(True, vis)]
            print(f"{name} layer {L}: index {index.tolist()} cost bound max {float(r['e_cost'].max()):.2e} reference-restatement "
                  f"{float(margin.max()):.2e}")
        assert list(ref_losses) == names, (list(ref_losses), names)
        mine = torch.stack([layers[L]["losses"][R.LOSS_ORDER.index(k)] for L in range(n_layers) for k in R.loss_names(True, vis)])
        vals = torch.stack([ref_losses[k].reshape(()) for k in names])
        assert all(v.dtype == torch.float32 for v in ref_losses.values())
        out[f"{name}_loss_names"], out[f"{name}_loss_values"] = np.asarray(names), vals.numpy()
        out[f"{name}_margin_losses"] = (vals.double() - mine).abs().numpy()
        print(f"{name}: num_boxes {num_boxes} losses {dict(zip(names, [round(float(v), 5) for v in vals]))} reference-restatement "
              f"{float((vals.double() - mine).abs().max()):.2e}")
    path = os.path.join(HERE, "criterion_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
