"""GPU: SetCriterion and its matcher (libtce_rvos_train.so) against the fp64 restatement within the bounds derived in
tests/_criterion.py, and against the reference's own matcher / criterion (tests/golden/criterion_cases.npz) within those bounds plus
the reference's recorded distance from the restatement.  Each figure is printed before it is asserted."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

import _criterion as R  # noqa: E402
from _util import load_npz, synth_frames  # noqa: E402

CASE = {c[0]: c for c in R.CASES}


def _crit(vis=False, K=1):
    from tce_rvos_amd.criterion import SetCriterion
    c = R.CONSTS
    return SetCriterion(K, {}, ["labels", "boxes", "masks"] + (["visible"] if vis else []),
                        focal_alpha=c["focal_alpha"], cost_class=c["cost_class"], cost_bbox=c["cost_bbox"], cost_giou=c["cost_giou"],
                        cost_mask=c["cost_mask"], cost_dice=c["cost_dice"], cost_vis=c["cost_vis"], masks=True, vis=vis)


def _cuda(outputs, targets, unaligned=False):
    def layer(o):
        d = {k: v.cuda() for k, v in o.items() if k != "aux_outputs"}
        if unaligned:  # the same values behind a base that is 4- but not 16-byte aligned
            pm = d["pred_masks"]
            buf = torch.empty(pm.numel() + 1, dtype=torch.float32, device="cuda")
            view = buf[1:].view(pm.shape)
            view.copy_(pm)
            assert view.is_contiguous() and view.data_ptr() % 16 == 4
            d["pred_masks"] = view
        return d
    out = layer(outputs)
    if "aux_outputs" in outputs:
        out["aux_outputs"] = [layer(a) for a in outputs["aux_outputs"]]
    return out, [{k: v.cuda() for k, v in t.items()} for t in targets]


@pytest.fixture(scope="module")
def runs():
    """Per case, computed once and left unchanged: the inputs, the restatement, the kernels' values and the loss dict"""
    cache = {}

    def get(name):
        if name not in cache:
            case = CASE[name]
            vis, K = case[8], case[5]
            outputs, targets = R.make_case(case)
            layers, num_boxes = R.restate(outputs, targets, R.CONSTS, masks=True, vis=vis)
            g_out, g_tg = _cuda(outputs, targets, unaligned=name in R.UNALIGNED)
            crit = _crit(vis, K)
            vals = crit.layer_values(g_out, g_tg)
            losses = crit(g_out, g_tg)
            torch.cuda.synchronize()
            cache[name] = dict(outputs=outputs, targets=targets, restated=layers, g_out=g_out, g_tg=g_tg, crit=crit, losses=losses,
                               vals=[{k: (None if v is None else v.cpu()) for k, v in d.items()} for d in vals])
        return cache[name]
    return get


@pytest.fixture(scope="module")
def fixture():
    return load_npz("criterion_cases.npz")


def _within(tag, got, want, bound):
    d = (got.double() - want.double()).abs()
    worst = float((d - bound).max())
    print(f"{tag}: max |d| {float(d.max()):.3e}  bound (min .. max) {float(torch.as_tensor(bound).min()):.3e} .. "
          f"{float(torch.as_tensor(bound).max()):.3e}")
    assert worst <= 0, (tag, float(d.max()), worst)


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_case_against_restatement_and_reference(runs, fixture, name):
    r = runs(name)
    case = CASE[name]
    vis = case[8]
    names = []
    for L, (v, want) in enumerate(zip(r["vals"], r["restated"])):
        _within(f"{name} L{L} sums", v["sums"], want["sums"], want["e_sums"])
        assert torch.equal(v["st"], want["st"])  # a count: exact
        _within(f"{name} L{L} cost", v["cost"], want["cost"], want["e_cost"])
        assert v["index"].tolist() == want["index"].tolist()
        _within(f"{name} L{L} parts", v["parts"], want["parts"], want["e_parts"])
        _within(f"{name} L{L} losses", v["losses"], want["losses"], want["e_losses"])
        # the reference itself: its cost column and match
        assert v["index"].tolist() == fixture[f"{name}_index{L}"].tolist()
        _within(f"{name} L{L} cost vs reference", v["cost"], torch.from_numpy(fixture[f"{name}_cost{L}"]),
                want["e_cost"] + torch.from_numpy(fixture[f"{name}_margin_cost{L}"]))
        names += [k + ("" if L == 0 else f"_{L - 1}") for k in R.loss_names(True, vis)]
    # the loss dict: the reference's keys in its order, 0-dim float32 device tensors, the reference's values
    assert list(r["losses"]) == names == list(fixture[f"{name}_loss_names"])
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in r["losses"].values())
    got = torch.stack([r["losses"][k].cpu() for k in names])
    e = torch.stack([r["restated"][L]["e_losses"][R.LOSS_ORDER.index(k)] for L in range(len(r["vals"])) for k in R.loss_names(True, vis)])
    _within(f"{name} loss dict vs reference", got, torch.from_numpy(fixture[f"{name}_loss_values"]),
            e + torch.from_numpy(fixture[f"{name}_margin_losses"]))
    mine = torch.stack([r["vals"][L]["losses"][R.LOSS_ORDER.index(k)] for L in range(len(r["vals"])) for k in R.loss_names(True, vis)])
    assert torch.equal(got, mine)  # forward() and layer_values() are the same launches


def test_matcher_return_format(runs):
    r = runs("c6")
    ind = r["crit"].matcher(r["g_out"], r["g_tg"])
    assert isinstance(ind, list) and len(ind) == 3
    for b, (src, tgt) in enumerate(ind):
        assert src.dtype == tgt.dtype == torch.int64 and src.is_cuda and tgt.is_cuda and tuple(src.shape) == tuple(tgt.shape) == (1,)
        assert int(src) == int(r["restated"][0]["index"][b]) and int(tgt) == 0


def test_duplicated_queries_tie_to_the_lower_index(runs):
    r = runs("c2")
    want = int(r["restated"][0]["index"][0])
    out = {k: torch.cat([v, v[:, :, want:want + 1], v], 2).contiguous() for k, v in r["g_out"].items()}  # Q = 5 -> 11
    vals = r["crit"].layer_values(out, r["g_tg"])[0]
    cost = vals["cost"].cpu()[0]
    assert torch.equal(cost[:5].view(torch.int32), cost[6:].view(torch.int32))          # bit-identical inputs, bit-identical costs
    assert cost[want].view(torch.int32) == cost[5].view(torch.int32) == cost[6 + want].view(torch.int32)
    assert torch.equal(cost[:5].view(torch.int32), r["vals"][0]["cost"][0].view(torch.int32))  # and independent of Q
    assert int(vals["index"]) == want                                                   # three equal minima: the lowest index


def test_two_runs_and_the_list_form_are_bit_identical(runs):
    r = runs("c6")
    again = r["crit"].layer_values(r["g_out"], r["g_tg"])[0]
    for k, v in again.items():
        assert torch.equal(v.cpu().view(torch.uint8), r["vals"][0][k].view(torch.uint8)), k
    per_clip = [{k: v[b:b + 1] for k, v in r["g_out"].items()} for b in range(3)]
    listed = r["crit"](per_clip, r["g_tg"])
    assert list(listed) == list(r["losses"])
    for k in listed:
        assert torch.equal(listed[k].view(torch.int32), r["losses"][k].view(torch.int32)), k


def test_capture_on_a_side_stream_replays_to_the_same_bits(runs, monkeypatch):
    """torch.cuda.graph on a side stream.  The captured program is a single chain: every launch of the call is issued to the one
    capturing stream (recorded below), the call waits on no other stream and records no event."""
    from tce_rvos_amd import train_ops
    r = runs("c8")  # three layers: six entry-point calls
    crit, out, tg = r["crit"], r["g_out"], r["g_tg"]
    side = torch.cuda.Stream()
    seen = []
    real = train_ops._stream

    def recording():
        seen.append(real())
        return seen[-1]

    monkeypatch.setattr(train_ops, "_stream", recording)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        losses = crit(out, tg)
    assert len(seen) == 6 and set(seen) == {side.cuda_stream}
    for v in losses.values():
        v.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for k, v in losses.items():
        assert torch.equal(v.view(torch.int32), r["losses"][k].view(torch.int32)), k
    g.replay()
    torch.cuda.synchronize()
    for k, v in losses.items():
        assert torch.equal(v.view(torch.int32), r["losses"][k].view(torch.int32)), k


def test_criterion_of_the_model_on_the_padded_clip():
    """criterion(model(...), targets) through build_model on the padded Swin-T fixture's clip: the values are the restatement's on
    the model's own outputs"""
    from tce_rvos_amd import build_model, load_synth_weights, nested_tensor_from_videos_list
    fx = load_npz("e2e_swin_t_padded.npz")
    T, hv, wv = (int(v) for v in fx["thw"])
    H, W = (int(v) for v in fx["padded_hw"])
    args = argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)
    model, crit, _ = build_model(args)
    model = model.cuda().eval()
    load_synth_weights(model, int(fx["weights_salt"]))
    model.repack()
    nt = nested_tensor_from_videos_list([synth_frames(T, hv, wv, int(fx["frames_seed"])).cuda()], size_divisibility=32)
    out = model.forward_features(nt.tensors[0], torch.from_numpy(fx["text_hidden"])[0].cuda(),
                                 torch.from_numpy(fx["text_pooled"])[0].cuda(), float(H), float(W), valid_hw=(hv, wv))
    g = torch.Generator().manual_seed(5)
    boxes = torch.cat([0.3 + 0.4 * torch.rand(T, 2, generator=g), 0.2 + 0.3 * torch.rand(T, 2, generator=g)], -1)
    masks = torch.zeros(T, hv, wv, dtype=torch.bool)
    masks[:, hv // 4:hv // 2, wv // 3:2 * wv // 3] = True
    valid = torch.tensor([1, 1, 0])
    targets = [{"masks": masks, "boxes": boxes * valid[:, None], "labels": torch.zeros(T, dtype=torch.int64), "valid": valid}]
    losses = crit(out, [{k: v.cuda() for k, v in targets[0].items()}])
    torch.cuda.synchronize()
    n_aux = len(out["aux_outputs"])
    assert n_aux == 3 and set(losses) == set(crit.weight_dict)
    host = {k: out[k].cpu() for k in ("pred_logits", "pred_boxes", "pred_masks")}
    host["aux_outputs"] = [{k: a[k].cpu() for k in ("pred_logits", "pred_boxes", "pred_masks")} for a in out["aux_outputs"]]
    c = dict(R.CONSTS)
    layers, _ = R.restate(host, [dict(targets[0], masks=masks.to(torch.uint8))], c, masks=True, vis=False)
    vals = crit.layer_values(out, [{k: v.cuda() for k, v in targets[0].items()}])
    for L, want in enumerate(layers):
        suffix = "" if L == 0 else f"_{L - 1}"
        srt = want["cost"][0].sort().values
        gap, bound = float(srt[1] - srt[0]), float(want["e_cost"].max())
        print(f"layer {L}: cost gap {gap:.3e} bound {bound:.3e}")
        assert gap > 10 * bound  # the clip's match does not hang on rounding, so index and losses are comparable
        _within(f"model L{L} cost", vals[L]["cost"].cpu(), want["cost"], want["e_cost"])
        assert vals[L]["index"].tolist() == want["index"].tolist()
        got = torch.stack([losses[k + suffix].cpu() for k in R.loss_names(True, False)])
        sel = [R.LOSS_ORDER.index(k) for k in R.loss_names(True, False)]
        _within(f"model L{L} losses", got, want["losses"][sel], want["e_losses"][sel])
