"""GPU: clip groups over a frame pool -- model.forward_indexed against each slot's own forward on the materialised clip, against
forward_group where the two programs coincide, its recorded launch program (the backbone sees the distinct frames only), and
video.run_video_windows(share="frames") against its planned forwards called by hand and against the default driver.

The bound between a group and its solo forwards is the project's group bound, tol(ref) = 2e-5 * max|ref| + 1e-6
(test_clip_group_matches_one_clip_at_a_time): the same kernels at another row count."""
import argparse
import math

import pytest
import torch
import torch.nn.functional as F

from _util import synth_frames

pytestmark = pytest.mark.gpu

GROUP_KEYS = ("pred_logits", "pred_boxes", "pred_masks", "memory", "reference_points")
PAD = 1


def _args(backbone):
    return argparse.Namespace(backbone=backbone, with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(backbone, salt=31):
        from tce_rvos_amd import build_model, load_synth_weights
        if backbone not in cache:
            m, _, _ = build_model(_args(backbone))
            m = m.cuda().eval()
            load_synth_weights(m, salt)
            m.repack()
            cache[backbone] = m
        return cache[backbone]
    return get


def tol(ref):
    return 2e-5 * float(ref.abs().max()) + 1e-6


def _tokens(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for n in lengths:
        t = torch.randint(3, 50000, (1, n), generator=g)
        t[0, 0], t[0, -1] = 0, 2
        rows.append(t)
    return rows


def _padded(rows):
    out = torch.full((len(rows), max(r.shape[1] for r in rows)), PAD, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :r.shape[1]] = r[0]
    return out


def _keep(o):
    return {k: o[k].clone() for k in GROUP_KEYS}


def _target(H, W):
    return [{"size": torch.tensor([H, W])}]


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


WINDOWS_6 = [(0, 0, 1, 2), (1, 2, 3, 4), (3, 4, 5, 5)]
# name: backbone, H, W, F, index, caption token lengths (one per slot), ragged
CASES = {
    "two captions x three windows": ("swin_t_p4w7", 96, 132, 6, WINDOWS_6 * 2, [9] * 2, False),
    "ragged captions": ("swin_t_p4w7", 96, 132, 6, WINDOWS_6, [6, 9, 9], True),
    "fused forms": ("swin_t_p4w7", 360, 640, 12, [(0, 0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9, 10)] * 2, [32] * 2, False),
    "resnet, one caption": ("resnet50", 96, 128, 5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 4)], [9], False),
    "video-swin": ("video_swin_t_p4w7", 96, 128, 6, [(0, 1, 2, 3), (0, 1, 2, 3), (2, 3, 4, 5)], [9, 9, 9], False),
    # 21 segments per level: the table is split over two copy launches (16 segments each)
    "two copy launches": ("swin_t_p4w7", 64, 96, 4, [(2, 0, 3), (1, 3, 0), (3, 1, 0)] * 2 + [(2, 0, 3)], [9], False),
}


def test_the_long_table_case_is_longer_than_one_launch_holds():
    from tce_rvos_amd.pipeline import pool_segments
    _, table = pool_segments(CASES["two copy launches"][4], [(16, 24)], [96], "frame")
    assert len(table[0]) == 21


def _case(name):
    """(pool, index, one [1, L] id tensor per slot, ragged): fewer captions than slots are spread caption-major"""
    backbone, H, W, Fp, index, lens, ragged = CASES[name]
    pool = synth_frames(Fp, H, W, 410 + len(name)).cuda()
    caps = _tokens(lens, 420 + len(name))
    per = len(index) // len(caps)
    rows = [caps[g // per] for g in range(len(index))]
    return backbone, H, W, pool, [tuple(t) for t in index], rows, ragged


# -------------------------------------------------------------------------------------------------- a group equals its solo forwards
@pytest.mark.parametrize("name", list(CASES))
def test_indexed_group_matches_one_clip_at_a_time(models, name):
    backbone, H, W, pool, index, rows, ragged = _case(name)
    model = models(backbone)
    ids = (_padded(rows) if ragged else torch.cat(rows, 0)).cuda()
    solo = {}
    for g, t in enumerate(index):  # one solo forward per distinct (clip, caption)
        k = (t, tuple(rows[g][0].tolist()))
        if k not in solo:
            solo[k] = _keep(model([pool[list(t)]], rows[g], _target(H, W)))
    runs = []
    for _ in range(3):  # eager, capture, replay
        outs = model.forward_indexed(pool, index, ids, _target(H, W), ragged=ragged)
        torch.cuda.synchronize()
        runs.append([_keep(o) for o in outs])
    assert len(outs) == len(index)
    assert set(outs[0]) == set(model([pool[list(index[0])]], rows[0], _target(H, W)))
    for g, t in enumerate(index):
        ref = solo[(t, tuple(rows[g][0].tolist()))]
        _hold(runs[0][g], ref, f"{name} slot {g}")
        _mask_signs_agree(runs[0][g], ref)
        for r in runs[1:]:
            for k in GROUP_KEYS:
                assert torch.equal(r[g][k], runs[0][g][k]), (g, k, "capture / replay != eager")


# -------------------------------------------------------------------------------------- where the program is forward_group's own
@pytest.mark.parametrize("backbone,H,W", [("swin_t_p4w7", 96, 132), ("resnet50", 96, 128)])
def test_identity_and_one_clip_groups_are_forward_group_bit_for_bit(models, backbone, H, W):
    model = models(backbone)
    G, Tc = 3, 3
    clips = [synth_frames(Tc, H, W, 500 + g).cuda() for g in range(G)]
    ids = torch.cat(_tokens([9] * G, 501), 0).cuda()
    for _ in range(3):  # eager, capture, replay -- of both
        want = model.forward_group(clips, ids, _target(H, W))
        got = model.forward_indexed(torch.cat(clips, 0), [tuple(range(g * Tc, (g + 1) * Tc)) for g in range(G)], ids, _target(H, W))
        torch.cuda.synchronize()
        for g in range(G):
            assert set(got[g]) == set(want[g])
            for k in GROUP_KEYS:
                assert torch.equal(got[g][k], want[g][k]), ("distinct clips", g, k)
    for _ in range(3):
        want = model.forward_group([clips[0]] * G, ids, _target(H, W))
        got = model.forward_indexed(clips[0], [tuple(range(Tc))] * G, ids, _target(H, W))
        torch.cuda.synchronize()
        for g in range(G):
            for k in GROUP_KEYS:
                assert torch.equal(got[g][k], want[g][k]), ("one clip, G captions", g, k)
    one = model.forward_indexed(clips[0], [(2, 0, 0)], ids[:1], _target(H, W))  # G = 1 goes to forward
    ref = model([clips[0][[2, 0, 0]]], ids[:1], _target(H, W))
    assert len(one) == 1 and all(torch.equal(one[0][k], ref[k]) for k in GROUP_KEYS)


# ------------------------------------------------------------------------------------------------- frames do not see each other
@pytest.mark.parametrize("backbone,H,W", [("swin_t_p4w7", 96, 132), ("resnet50", 96, 128)])
def test_a_pool_frame_reaches_only_the_slots_that_name_it(models, backbone, H, W):
    model = models(backbone)
    pool = synth_frames(6, H, W, 600).cuda()
    index = WINDOWS_6 * 2
    ids = torch.cat([r for r in _tokens([9, 9], 601) for _ in WINDOWS_6], 0).cuda()
    a = [_keep(o) for o in model.forward_indexed(pool, index, ids, _target(H, W))]
    other = pool.clone()
    other[5] = synth_frames(1, H, W, 602).cuda()[0]
    b = [_keep(o) for o in model.forward_indexed(other, index, ids, _target(H, W))]
    for g, t in enumerate(index):
        same = all(torch.equal(a[g][k], b[g][k]) for k in GROUP_KEYS)
        assert same == (5 not in t), (g, t)


# --------------------------------------------------------------------------------------------------------- the launch program
def _recorded(model, pool, index, ids, H, W):
    seen = {}

    def observe(when, res, rec):
        if when == "after":
            seen["launches"] = [(L.name, int((L.writes[:, 1] - L.writes[:, 0]).sum())) for L in rec.launches]
    rep = model.hazard_check(pool, ids, (H, W), index=index, observe=observe)
    return rep, seen["launches"]


@pytest.mark.parametrize("name", ["two captions x three windows", "resnet, one caption", "video-swin"])
def test_the_backbone_sees_each_distinct_frame_once_and_the_program_is_race_free(models, name):
    backbone, H, W, pool, index, rows, _ = _case(name)
    model = models(backbone)
    rep, launches = _recorded(model, pool, index, torch.cat(rows, 0).cuda(), H, W)
    assert rep.clean, str(rep)
    slots = len(index) * len(index[0])
    if backbone == "resnet50":
        U = len({f for t in index for f in t})
        first = [b for n, b in launches if n == "tce_resnet_stem_f32"]
        per_frame = ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * 64 * 4
    else:
        U = len(set(index)) * len(index[0]) if backbone.startswith("video") else len({f for t in index for f in t})
        first = [b for n, b in launches if n == "tce_patch_embed_f32"]
        per_frame = ((H + 3) // 4) * ((W + 3) // 4) * model.cfg.embed_dim * 4
    assert U < slots
    assert first == [U * per_frame], (first, U, per_frame, slots)
    copies = sum(1 for n, _ in launches if n == "tce_copy_segments")
    assert copies >= 4  # one gather per backbone stage at least
    if backbone.startswith("video"):
        n3d = sum(1 for n, _ in launches if n == "tce_window_attn3d_f32")
        assert n3d == sum(model.cfg.depths) * len(set(index)), (n3d, model.cfg.depths, len(set(index)))


def test_an_identity_index_launches_no_gather(models):
    model = models("swin_t_p4w7")
    H, W = 96, 132
    pool = synth_frames(4, H, W, 700).cuda()
    ids = torch.cat(_tokens([9, 9], 701), 0).cuda()
    index = [(0, 1), (2, 3)]
    _, launches = _recorded(model, pool, index, ids, H, W)
    _, plain = _recorded(model, pool, [(0, 1), (1, 2)], ids, H, W)
    n_id = sum(1 for n, _ in launches if n == "tce_copy_segments")
    n_g = sum(1 for n, _ in plain if n == "tce_copy_segments")
    assert n_g == n_id + 4, (n_id, n_g)  # four stages, one merged table each


# ------------------------------------------------------------------------------------------------------------------ the driver
N, DH, DW, ORIGIN, NF = 13, 96, 132, (120, 165), 3
KEYS = ("pred_logits", "pred_boxes", "reference_points")
DRIVER_LENS = [9, 9, 6]


@pytest.fixture(scope="module")
def video():
    return synth_frames(N, DH, DW, 810).cuda()


def _frames_by_hand(model, frames, toks, plan, forwards, mixed):
    """The planned share="frames" forwards through model.forward_indexed and ops.select_window_masks, one call each"""
    from tce_rvos_amd import ops
    from tce_rvos_amd.video import window_pool
    res = {}
    for caps, wins in forwards:
        pool_ids, index = window_pool(plan, wins, len(caps))
        rows = [toks[i] for i in caps for _ in wins]
        if len(rows) == 1:
            tok, kw = rows[0], {}
        elif mixed:
            tok, kw = _padded(rows).cuda(), {"ragged": True}
        else:
            tok, kw = torch.cat(rows, 0).cuda(), {}
        outs = model.forward_indexed(frames[pool_ids], index, tok, _target(DH, DW), **kw)
        for (i, w), out in zip([(i, w) for i in caps for w in wins], outs):
            _, first, count, _ = plan[w]
            m, b = ops.select_window_masks(out["pred_logits"][0], out["pred_masks"][0], ORIGIN, first, count, 0.5)
            q = int(b)
            res[(i, w)] = {"masks": m, "best": q, **{k: out[k][0][first:first + count, q].clone() for k in KEYS}}
    return res


def _hold_to_hand(got, hand, i, plan):
    assert tuple(got["masks"].shape) == (N,) + ORIGIN and got["masks"].dtype == torch.uint8
    assert got["windows"] == plan
    for w, (_, _, count, lo) in enumerate(plan):
        want = hand[(i, w)]
        assert int(got["best_query"][w]) == want["best"], (i, w)
        assert torch.equal(got["masks"][lo:lo + count], want["masks"]), (i, w)
        for k in KEYS:
            assert torch.equal(got[k][lo:lo + count], want[k]), (i, w, k)


@pytest.mark.parametrize("e,mixed,last", [(0, False, "short"), (1, False, "short"), (1, True, "short"), (1, False, "shifted")])
def test_frame_sharing_driver_is_its_planned_forwards_called_by_hand(models, video, e, mixed, last):
    from tce_rvos_amd.video import plan_window_forwards, plan_windows, run_video_windows
    model = models("swin_t_p4w7")
    toks = _tokens(DRIVER_LENS, 811)
    plan = plan_windows(N, NF, e, last)
    forwards = plan_window_forwards(DRIVER_LENS, plan, mixed_lengths=mixed, share="frames", max_pairs=6)
    assert sorted((i, w) for c, ws in forwards for i in c for w in ws) == [(i, w) for i in range(3) for w in range(len(plan))]
    got = run_video_windows(model, video, toks, ORIGIN, NF, e, last=last, mixed_lengths=mixed, share="frames", max_pairs=6)
    torch.cuda.synchronize()
    assert isinstance(got, list) and len(got) == 3
    hand = _frames_by_hand(model, video, toks, plan, forwards, mixed)
    for i in range(3):
        _hold_to_hand(got[i], hand, i, plan)
        assert 0 < int(got[i]["masks"].sum()) < got[i]["masks"].numel()


@pytest.mark.parametrize("e", [0, 1])
def test_frame_sharing_driver_against_the_default_driver(models, video, e):
    """Both drivers run the same (caption, window) pairs in groups of other shapes, so their mask logits differ by the group
    round-off, tol = 2e-5 * max|pred_masks| + 1e-6 per forward.  A mask pixel may differ only where the up-sampled logit of the
    DEFAULT driver's forward (bilinear: a convex combination, so the bound carries over) lies within tol of logit(threshold) = 0;
    that set must be below 1e-4 of the pixels, and the best queries must agree.  Seeds (frames 810, captions 811) chosen from the
    CPU oracle's solo forwards (oracle.tce_oracle.forward per caption and window, F.interpolate of the best query's kept planes):
    9 (f_extra 0) and 5 (f_extra 1) of 772200 pixels lie within the band, and the best query leads by at least 3.4e-4 in mean
    score.  The set's size on the GPU is printed before the assertion.  The per-frame rows of the best query (logits, boxes,
    reference points) are held to 2 * tol: each driver is within tol of the solo forward."""
    from tce_rvos_amd.video import plan_window_forwards, plan_windows, run_video_windows
    model = models("swin_t_p4w7")
    toks = _tokens(DRIVER_LENS, 811)
    plan = plan_windows(N, NF, e)
    want = run_video_windows(model, video, toks, ORIGIN, NF, e)
    got = run_video_windows(model, video, toks, ORIGIN, NF, e, share="frames")
    torch.cuda.synchronize()
    edge = math.log(0.5 / 0.5)
    near = [torch.zeros((N,) + ORIGIN, dtype=torch.bool, device="cuda") for _ in toks]
    for caps, wins in plan_window_forwards(DRIVER_LENS, plan):  # the default driver's forwards, by hand
        clips = [video[list(plan[w][0])] for w in wins]
        if len(caps) == 1:
            tok = toks[caps[0]] if len(wins) == 1 else toks[caps[0]].cuda().expand(len(wins), -1).contiguous()
            outs, pairs = model.forward_group(clips, tok, _target(DH, DW)), [(caps[0], w) for w in wins]
        else:
            outs = model.forward_group(clips * len(caps), torch.cat([toks[i] for i in caps], 0).cuda(), _target(DH, DW))
            pairs = [(i, wins[0]) for i in caps]
        for (i, w), out in zip(pairs, outs):
            _, first, count, lo = plan[w]
            pm = out["pred_masks"][0]
            q = int(want[i]["best_query"][w])
            up = F.interpolate(pm[first:first + count, q][None], size=ORIGIN, mode="bilinear", align_corners=False)[0]
            near[i][lo:lo + count] = (up - edge).abs() <= tol(pm)
    total = sum(int(m.numel()) for m in near)
    n_near = sum(int(m.sum()) for m in near)
    n_diff = sum(int((g["masks"] != w_["masks"]).sum()) for g, w_ in zip(got, want))
    print(f"f_extra {e}: {n_near} of {total} pixels within the band, {n_diff} mask pixels differ")
    assert n_near < 1e-4 * total, (n_near, total)
    for i in range(3):
        assert torch.equal(got[i]["best_query"], want[i]["best_query"]), i
        assert not bool(((got[i]["masks"] != want[i]["masks"]) & ~near[i]).any()), i
        for k in KEYS:
            assert float((got[i][k] - want[i][k]).abs().max()) <= 2 * tol(want[i][k]), (i, k)
