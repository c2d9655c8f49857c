"""GPU: A2D-Sentences / JHMDB-Sentences clip groups -- model.forward_group with per-clip valid_indices (one annotated frame per clip)
against each clip's own forward(..., valid_indices), the reference's fixture, the hazard checker, and video.run_annotated_frames.

The bound between a group and its solo forwards is the project's group bound, tol(ref) = 2e-5 * max|ref| + 1e-6
(test_clip_group_matches_one_clip_at_a_time): the same kernels at another row count."""
import argparse

import pytest
import torch

from oracle import tce_oracle as O
from _util import load_npz, synth_frames

pytestmark = pytest.mark.gpu

GROUP_KEYS = ("pred_logits", "pred_boxes", "pred_masks", "memory", "reference_points")
PAD = 1


def _args(backbone):
    return argparse.Namespace(backbone=backbone, with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(backbone, salt):
        from tce_rvos_amd import build_model, load_synth_weights
        if backbone not in cache:
            m, _, _ = build_model(_args(backbone))
            cache[backbone] = m.cuda().eval()
        m = cache[backbone]
        load_synth_weights(m, salt)
        m.repack()
        return m
    return get


def tol(ref):
    return 2e-5 * float(ref.abs().max()) + 1e-6


def _inputs(G, T, H, W, L, seed=70):
    clips = [synth_frames(T, H, W, seed + i).cuda() for i in range(G)]
    g = torch.Generator().manual_seed(seed)
    return clips, torch.randint(3, 50000, (G, L), generator=g).cuda()


def _targets(H, W, idx):
    return [{"size": torch.tensor([H, W]), "valid_indices": torch.tensor(int(i))} for i in idx]


def _keep(o):
    return {k: o[k].clone() for k in GROUP_KEYS}


def _solos(model, clips, ids, H, W, idx):
    return [_keep(model([clips[g]], ids[g][None] if ids[g].dim() == 1 else ids[g], _targets(H, W, idx[g:g + 1]))) for g in range(len(clips))]


def _hold(got, ref, what):
    """shapes equal, values within tol(ref); prints the figures before it asserts"""
    for k in GROUP_KEYS:
        assert got[k].shape == ref[k].shape, (what, k, tuple(got[k].shape), tuple(ref[k].shape))
        err, t = float((got[k] - ref[k]).abs().max()), tol(ref[k])
        print(f"{what} {k}: max|diff| {err:.3e} (tol {t:.3e})")
        assert err <= t, (what, k, err, t)


def _mask_signs_agree(got, ref):
    pm = ref["pred_masks"]
    sure = pm.abs() > tol(pm)
    a, b = (pm > 0) & sure, (got["pred_masks"] > 0) & sure
    inter, union = (a & b).sum().item(), (a | b).sum().item()
    assert union == 0 or inter / union > 0.9999, inter / union


# ------------------------------------------------------------------------------------------------------- group equals solo
@pytest.mark.parametrize("backbone,G,T,H,W,L,idx", [("swin_t_p4w7", 3, 3, 96, 132, 9, (1, 0, 2)),
                                                    ("video_swin_t_p4w7", 2, 4, 96, 128, 9, (3, 0)),
                                                    ("resnet50", 4, 3, 96, 128, 9, (0, 2, 1, 1)),
                                                    ("swin_t_p4w7", 2, 5, 64, 96, 40, (4, 4))])    # captions above 32 tokens
def test_single_frame_group_matches_one_clip_at_a_time(models, backbone, G, T, H, W, L, idx):
    model = models(backbone, 31)
    clips, ids = _inputs(G, T, H, W, L)
    solo = _solos(model, clips, ids, H, W, idx)
    runs = []
    for _ in range(3):  # eager, capture, replay
        outs = model.forward_group(clips, ids, _targets(H, W, idx))
        torch.cuda.synchronize()
        runs.append([_keep(o) for o in outs])
    assert len(runs[0]) == G
    for g in range(G):
        assert tuple(runs[0][g]["pred_masks"].shape[:3]) == (1, 1, 5) and tuple(runs[0][g]["pred_logits"].shape) == (1, 1, 5, 1)
        assert set(outs[g]) == set(model([clips[g]], ids[g:g + 1], _targets(H, W, idx[g:g + 1])))
        _hold(runs[0][g], solo[g], f"{backbone} clip {g}")
        for r in runs[1:]:
            for k in GROUP_KEYS:
                assert torch.equal(r[g][k], runs[0][g][k]), (g, k, "replay != eager")
        _mask_signs_agree(runs[0][g], solo[g])


def test_shared_single_frame_group_runs_the_backbone_once(models):
    """The same tensor 3 times (3 expressions of one A2D clip), indices (0, 1, 1): each result is its solo forward's; race-free."""
    model = models("swin_t_p4w7", 31)
    T, H, W, idx = 3, 96, 132, (0, 1, 1)
    clips, _ = _inputs(1, T, H, W, 9)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, 50000, (3, 9), generator=g).cuda()
    solo = _solos(model, [clips[0]] * 3, ids, H, W, idx)
    runs = []
    for _ in range(3):
        outs = model.forward_group([clips[0]] * 3, ids, _targets(H, W, idx))
        torch.cuda.synchronize()
        runs.append([_keep(o) for o in outs])
    for i in range(3):
        _hold(runs[0][i], solo[i], f"shared caption {i}")
        for k in GROUP_KEYS:
            assert torch.equal(runs[1][i][k], runs[0][i][k]) and torch.equal(runs[2][i][k], runs[0][i][k]), (i, k)
    assert not torch.equal(runs[0][1]["pred_masks"], runs[0][2]["pred_masks"])  # same frame, another caption
    rep = model.hazard_check(clips[0], ids, (H, W), groups=3, shared=True, select=idx)
    assert rep.clean, str(rep)


def test_group_of_two_from_text_features_matches_the_reference_fixture(models):
    """The reference's own single-frame run (e2e_swin_t_valid_idx.npz) as clip 0 of a group of 2 whose clip 1 is other frames and
    another index: clip 0 meets the tolerances of test_valid_indices_single_frame_path_matches_reference."""
    fx = load_npz("e2e_swin_t_valid_idx.npz")
    T, H, W = (int(v) for v in fx["thw"])
    vi = int(fx["valid_index"])
    other = (vi + 1) % T
    model = models("swin_t_p4w7", int(fx["weights_salt"]))
    frames = torch.cat([synth_frames(T, H, W, int(fx["frames_seed"])), synth_frames(T, H, W, int(fx["frames_seed"]) + 17)], 0).cuda()
    hid, pooled = torch.from_numpy(fx["text_hidden"])[0].cuda(), torch.from_numpy(fx["text_pooled"])[0].cuda()
    runs = [model.forward_features(frames, torch.cat([hid, hid], 0), torch.stack([pooled, pooled], 0), float(H), float(W),
                                   groups=2, select=(vi, other)) for _ in range(3)]   # eager, capture, replay
    torch.cuda.synchronize()
    assert all(len(r) == 2 for r in runs)
    out = runs[0][0]
    assert tuple(out["pred_masks"].shape) == (1, 1, 5, 18, 25) and tuple(out["memory"].shape) == tuple(fx["out_memory"].shape)
    for k, t in (("pred_logits", 2e-3), ("pred_boxes", 1e-4), ("reference_points", 1e-4), ("memory", 1e-3)):
        d = (out[k].cpu() - torch.from_numpy(fx["out_" + k])).abs().max().item()
        print(f"{k}: max|diff| vs the reference {d:.3e} (bound {t})")
        assert d < t, k
    ref = torch.from_numpy(fx["out_pred_masks"])
    d = (out["pred_masks"].cpu() - ref).abs().max().item()
    print(f"pred_masks: max|diff| vs the reference {d:.3e} (bounds 5e-3 and {2e-5 * float(ref.abs().max()):.3e})")
    assert d < 5e-3 and d <= 2e-5 * float(ref.abs().max()), d
    assert O.mask_iou(out["pred_masks"].cpu() > 0, ref > 0) > 1 - 1e-3
    for i in range(3):
        assert (out["aux_outputs"][i]["pred_masks"].cpu() - torch.from_numpy(fx[f"aux{i}_pred_masks"])).abs().max().item() < 5e-3
    for r in runs[1:]:
        for g in range(2):
            for k in GROUP_KEYS:
                assert torch.equal(r[g][k], runs[0][g][k]), (g, k)
    assert not torch.equal(runs[0][0]["pred_masks"], runs[0][1]["pred_masks"])
    with pytest.raises(IndexError):
        model.forward_features(frames, torch.cat([hid, hid], 0), torch.stack([pooled, pooled], 0), float(H), float(W), groups=2, select=(vi, T))


def test_single_frame_group_clips_do_not_see_each_other(models):
    """Changing clip 1's frames, caption and index leaves clip 0 bit-identical."""
    model = models("swin_t_p4w7", 31)
    T, H, W = 3, 96, 132
    clips, ids = _inputs(2, T, H, W, 9)
    a = _keep(model.forward_group(clips, ids, _targets(H, W, (1, 0)))[0])
    other, ids2 = _inputs(2, T, H, W, 9, seed=123)
    b = _keep(model.forward_group([clips[0], other[1]], torch.cat([ids[:1], ids2[1:]], 0), _targets(H, W, (1, 2)))[0])
    for k in GROUP_KEYS:
        assert torch.equal(a[k], b[k]), k


def test_ragged_single_frame_group_matches_each_pair_alone(models):
    model = models("swin_t_p4w7", 31)
    T, H, W, lens, idx = 3, 96, 132, (5, 9), (2, 0)
    clips, _ = _inputs(2, T, H, W, 9, seed=60)
    g = torch.Generator().manual_seed(61)
    ids = torch.full((2, max(lens)), PAD, dtype=torch.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = torch.randint(3, 50000, (n,), generator=g)
        ids[i, 0], ids[i, n - 1] = 0, 2
    ids = ids.cuda()
    solo = _solos(model, clips, [ids[i:i + 1, :n] for i, n in enumerate(lens)], H, W, idx)
    outs = model.forward_group(clips, ids, _targets(H, W, idx), ragged=True)
    torch.cuda.synchronize()
    for i in range(2):
        _hold(_keep(outs[i]), solo[i], f"ragged clip {i} ({lens[i]} tokens)")


def test_every_index_tuple_has_its_own_graph_within_the_cache_bound(models):
    model = models("swin_t_p4w7", 31)
    T, H, W = 3, 96, 132
    clips, ids = _inputs(2, T, H, W, 9, seed=90)
    tuples = ((0, 2), (2, 1))
    solo = {idx: _solos(model, clips, ids, H, W, idx) for idx in tuples}
    before = {k for k in model._graphs}
    for _ in range(2):  # eager sighting, capture
        for idx in tuples:
            model.forward_group(clips, ids, _targets(H, W, idx))
    torch.cuda.synchronize()
    new = [k for k in model._graphs if k not in before and k[0] == "group"]
    assert sorted(k[-1] for k in new) == sorted(("select", idx) for idx in tuples), new
    n = len(model._graphs)
    for idx in tuples:  # replays, interleaved: each graph gathers its own frames
        outs = model.forward_group(clips, ids, _targets(H, W, idx))
        torch.cuda.synchronize()
        for g in range(2):
            _hold(_keep(outs[g]), solo[idx][g], f"replay of {idx} clip {g}")
    assert len(model._graphs) == n <= model.max_graphs
    # more tuples than the cache holds: the bound stands
    for idx in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 2)):
        for _ in range(2):
            model.forward_group(clips, ids, _targets(H, W, idx))
    torch.cuda.synchronize()
    assert len(model._graphs) <= model.max_graphs


@pytest.mark.parametrize("backbone,G,T,H,W,idx", [("swin_t_p4w7", 2, 3, 96, 132, (2, 0)), ("resnet50", 4, 3, 96, 128, (0, 2, 1, 1))])
def test_single_frame_group_launch_program_is_race_free(models, backbone, G, T, H, W, idx):
    model = models(backbone, 5)
    clips, ids = _inputs(G, T, H, W, 9)
    rep = model.hazard_check(torch.cat(clips, 0), ids, (H, W), groups=G, select=idx)
    assert rep.clean, str(rep)


def test_errors(models):
    model = models("swin_t_p4w7", 31)
    T, H, W = 3, 96, 132
    clips, ids = _inputs(2, T, H, W, 9)
    mixed = [{"size": torch.tensor([H, W]), "valid_indices": torch.tensor(1)}, {"size": torch.tensor([H, W])}]
    with pytest.raises(ValueError, match="valid_indices"):
        model.forward_group(clips, ids, mixed)
    with pytest.raises(ValueError, match="valid_indices"):
        model.forward_group(clips, ids, mixed[::-1])
    with pytest.raises(IndexError):
        model.forward_group(clips, ids, _targets(H, W, (0, T)))
    with pytest.raises(IndexError):
        model.forward_group(clips, ids, _targets(H, W, (-1, 0)))
    # device tensors and plain ints are read alike
    a = model.forward_group(clips, ids, [{"size": torch.tensor([H, W]), "valid_indices": torch.tensor([i]).cuda()} for i in (1, 2)])
    b = model.forward_group(clips, ids, [{"size": torch.tensor([H, W]), "valid_indices": i} for i in (1, 2)])
    for k in GROUP_KEYS:
        assert torch.equal(a[0][k], b[0][k]) and torch.equal(a[1][k], b[1][k])
    one = model.forward_group(clips[:1], ids[:1], _targets(H, W, (2,)))   # G = 1 delegates to forward
    ref = model([clips[0]], ids[:1], _targets(H, W, (2,)))
    assert len(one) == 1 and torch.equal(one[0]["pred_masks"], ref["pred_masks"])


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_run_annotated_frames_is_the_planned_groups_called_by_hand(models):
    from tce_rvos_amd.postprocess import A2DSentencesPostProcess
    from tce_rvos_amd.video import plan_single_frame_groups, run_annotated_frames
    model = models("swin_t_p4w7", 31)
    T = 3
    shapes = [(96, 132), (96, 128), (96, 132), (96, 132), (96, 128)]
    index = [1, 0, 1, 0, 0]
    origs = [(120, 165), (96, 128), (111, 150), (60, 80), (200, 260)]
    g = torch.Generator().manual_seed(7)
    samples = [{"clip": synth_frames(T, h, w, 300 + i).cuda(), "caption": torch.randint(3, 50000, (1, 9), generator=g),
                "valid_index": vi, "orig_size": og} for i, ((h, w), vi, og) in enumerate(zip(shapes, index, origs))]
    post = A2DSentencesPostProcess(grouped=True)
    got = run_annotated_frames(model, samples, post, max_group=2)
    torch.cuda.synchronize()
    plan = plan_single_frame_groups([tuple(s["clip"].shape) for s in samples], index, [9] * 5, max_group=2)
    assert plan == [[0, 2], [1, 4], [3]]
    assert len(got) == 5
    raw = run_annotated_frames(model, samples, None, max_group=2)
    for grp in plan:
        h, w = shapes[grp[0]]
        outs = model.forward_group([samples[i]["clip"] for i in grp], torch.cat([samples[i]["caption"] for i in grp], 0).cuda(),
                                   [{"size": torch.tensor([h, w]), "valid_indices": index[i]} for i in grp])
        want = post(outs, [origs[i] for i in grp], [(h, w)] * len(grp))
        for i, o, r in zip(grp, outs, want):
            assert set(got[i]) == {"scores", "masks", "rle_masks"} and tuple(got[i]["masks"].shape) == (5, 1) + origs[i]
            assert torch.equal(got[i]["scores"], r["scores"]) and torch.equal(got[i]["masks"], r["masks"]), i
            assert got[i]["rle_masks"] == r["rle_masks"], i
            for k in GROUP_KEYS:
                assert torch.equal(raw[i][k], o[k]), (i, k)
