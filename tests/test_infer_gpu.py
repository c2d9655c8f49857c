"""GPU: the split driver (infer.run_split) against the sequential hand loop over the same calls -- Pillow decode, .cuda(), the same
front-end, the same driver function, png.mask_pngs / label_pngs -- file for file, byte for byte, in every mode, without read-ahead
and with staging and device buffers reused several times."""
import argparse
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

H, W, SIZE = 48, 72, 32
LENGTHS = {"kite": 4, "boat": 2, "swan": 6}
EXPRESSIONS = {"kite": {"0": "a kite", "1": "the red kite that flies over the beach"},
               "boat": {"2": "a boat", "0": "the small boat on the left", "1": "a white boat which moves slowly away from the shore"},
               "swan": {"0": "the swan", "1": "a swan that swims behind the other swan"}}
VIDEO_KW = {"clip_size": 4, "mixed_lengths": True}
WINDOW_KW = {"num_frames": 2, "f_extra": 1}
OBJECT_CAPTIONS = {"0": "a swan", "1": "the swan on the left", "2": "a bird that swims", "3": "the white swan near the shore of the lake"}


@pytest.fixture(scope="module")
def model():
    from tce_rvos_amd import build_model, load_synth_weights
    args = argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)
    m, _, _ = build_model(args)
    m = m.cuda().eval()
    load_synth_weights(m, 37)
    m.repack()
    return m


@pytest.fixture(scope="module")
def frontend():
    from tce_rvos_amd.frontend import ClipFrontEnd
    return ClipFrontEnd(size=SIZE)


def _frame(rng, k):
    """blobs that move with k over a smooth ground: JPEG-friendly, different in every frame and video"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([96 + 64 * np.sin(x / 11 + rng.uniform(0, 6)), 96 + 64 * np.cos(y / 7 + rng.uniform(0, 6)), 128 + 0 * x], -1)
    for _ in range(3):
        cy, cx, r = rng.uniform(8, H - 8), rng.uniform(8, W - 8) + 3 * k, rng.uniform(5, 12)
        img[(y - cy) ** 2 + (x - cx) ** 2 < r * r] = rng.uniform(0, 255, 3)
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    from tce_rvos_amd.infer import VideoJob
    root = tmp_path_factory.mktemp("split")
    rng = np.random.default_rng(5)
    jobs = []
    for name, n in LENGTHS.items():
        os.makedirs(root / name)
        names = ["%05d" % (5 * k) for k in range(n)]
        paths = [str(root / name / (f + ".jpg")) for f in names]
        for k, p in enumerate(paths):
            Image.fromarray(_frame(rng, k)).save(p, quality=90)
        jobs.append(VideoJob(name, paths, names, dict(EXPRESSIONS[name])))
    return jobs


def _decoded(job):
    return np.stack([np.asarray(Image.open(p).convert("RGB")) for p in job.frame_paths])


def _hand(model, frontend, jobs, call, key, to_files):
    """the sequential loop: {video: [(planes on the host, [file bytes]) per result]}"""
    out = {}
    for job in jobs:
        u8 = _decoded(job)
        frames = frontend(torch.from_numpy(u8).cuda())
        res = call(model, frames, list(job.expressions.values()), tuple(u8.shape[1:3]))
        out[job.name] = [(r[key].cpu().numpy(), to_files(r[key])) for r in res]
        torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def hand_video(model, frontend, split):
    from tce_rvos_amd import png, video
    want = _hand(model, frontend, split, lambda m, f, c, hw: video.run_video_expressions(m, f, c, hw, **VIDEO_KW), "masks", png.mask_pngs)
    planes = [p for v in want.values() for p, _ in v]
    assert all(p.shape[1:] == (H, W) and p.dtype == np.uint8 for p in planes)
    share = [float(p.mean()) for p in planes]
    print("foreground share per (video, expression):", [round(s, 3) for s in share])
    assert any(0 < s < 1 for s in share), "every mask of the hand loop is empty or full: the comparison would show nothing"
    return want


def _check_expression_tree(out, jobs, want, source=None):
    files = 0
    for job in jobs:
        per_exp = want[(source or {}).get(job.name, job.name)]
        assert len(per_exp) == len(job.expressions)
        for (masks, blobs), exp_id in zip(per_exp, job.expressions):
            assert sorted(os.listdir(os.path.join(out, job.name, exp_id))) == sorted(f + ".png" for f in job.frame_names)
            for k, f in enumerate(job.frame_names):
                path = os.path.join(out, job.name, exp_id, f + ".png")
                with open(path, "rb") as fh:
                    assert fh.read() == blobs[k], path
                im = Image.open(path)
                assert im.mode == "L" and np.array_equal(np.asarray(im), masks[k] * 255), path
                files += 1
    assert sorted(os.listdir(out)) == sorted(j.name for j in jobs)
    return files


def _afterwards(base):
    from tce_rvos_amd import ops
    assert threading.active_count() == base
    torch.cuda.synchronize()
    ops.check_range(torch.device("cuda", torch.cuda.current_device()))


@pytest.mark.parametrize("workers,depth", [(4, 2), (1, 0)])
def test_video_mode_writes_the_hand_loop_s_files(model, frontend, split, hand_video, tmp_path, workers, depth):
    from tce_rvos_amd.infer import run_split
    base = threading.active_count()
    out = str(tmp_path / "out")
    res = run_split(model, split, out, mode="video", frontend=frontend, driver_kwargs=VIDEO_KW, workers=workers, depth=depth)
    files = _check_expression_tree(out, split, hand_video)
    assert (res["videos"], res["frames"], res["pairs"], res["files"]) == (3, 12, 7, files) and files == 4 * 2 + 2 * 3 + 6 * 2
    tl = res["timeline"]
    first_forward = tl.index(next(ev for ev in tl if ev[:3] == ("forward", 0, "begin")))
    for v in range(depth + 1):
        assert tl.index(next(ev for ev in tl if ev[:3] == ("decode", v, "begin"))) < first_forward
    _afterwards(base)


def test_windows_mode_writes_the_hand_loop_s_files(model, frontend, split, tmp_path):
    from tce_rvos_amd import png, video
    from tce_rvos_amd.infer import run_split
    base = threading.active_count()
    want = _hand(model, frontend, split, lambda m, f, c, hw: video.run_video_windows(m, f, c, hw, **WINDOW_KW), "masks", png.mask_pngs)
    out = str(tmp_path / "out")
    res = run_split(model, split, out, mode="windows", frontend=frontend, driver_kwargs=WINDOW_KW, workers=4, depth=2)
    assert res["files"] == _check_expression_tree(out, split, want)
    _afterwards(base)


@pytest.mark.parametrize("sets", ["one map", "annotators"])
def test_objects_mode_writes_the_hand_loop_s_label_maps(model, frontend, split, tmp_path, sets):
    from tce_rvos_amd import png, video
    from tce_rvos_amd.infer import VideoJob, run_split
    base = threading.active_count()
    palette = bytes(np.random.default_rng(11).integers(0, 256, 768, dtype=np.uint8))
    swan = split[2]
    job = VideoJob("swan", swan.frame_paths, swan.frame_names, dict(OBJECT_CAPTIONS))
    kw = {"clip_size": 4, "mixed_lengths": True}
    object_sets = None if sets == "one map" else video.davis_annotator_sets(4)
    want = _hand(model, frontend, [job], lambda m, f, c, hw: video.run_video_objects(m, f, c, hw, object_sets=object_sets, **kw),
                 "labels", lambda planes: png.label_pngs(planes, palette))["swan"]
    assert len(want) == (1 if sets == "one map" else 4)
    print("labels in use:", [sorted(np.unique(labels).tolist()) for labels, _ in want])
    out = str(tmp_path / "out")
    if sets == "annotators":
        kw["object_sets"] = video.davis_annotator_sets  # resolved per video from its expression count
    res = run_split(model, [job], out, mode="objects", palette=palette, frontend=frontend, driver_kwargs=kw, workers=4, depth=2)
    assert sorted(os.listdir(out)) == [f"anno_{k}" for k in range(len(want))]
    for k, (labels, blobs) in enumerate(want):
        d = os.path.join(out, f"anno_{k}", "swan")
        assert sorted(os.listdir(d)) == ["%05d.png" % f for f in range(6)]
        for f in range(6):
            with open(os.path.join(d, "%05d.png" % f), "rb") as fh:
                assert fh.read() == blobs[f], (k, f)
            im = Image.open(os.path.join(d, "%05d.png" % f))
            assert im.mode == "P" and np.array_equal(np.asarray(im), labels[f]), (k, f)
    assert (res["videos"], res["frames"], res["pairs"], res["files"]) == (1, 6, 4, 6 * len(want))
    _afterwards(base)


def test_reused_buffers_hold_the_right_video(model, frontend, split, hand_video, tmp_path):
    """Five videos of 4, 2, 6, 6 and 4 frames through depth = 1: two staging buffers and two device buffers, each reused (and
    regrown) while the video before is still being read.  An upload that overwrote frames the front-end had not read yet, or a
    staging buffer decoded into before its copy was done, would put one video's pixels under another's masks."""
    from tce_rvos_amd.infer import VideoJob, run_split
    base = threading.active_count()
    again = {"swan2": "swan", "kite2": "kite"}
    jobs = list(split) + [VideoJob(new, split[i].frame_paths, split[i].frame_names, split[i].expressions)
                          for new, i in (("swan2", 2), ("kite2", 0))]
    out = str(tmp_path / "out")
    res = run_split(model, jobs, out, mode="video", frontend=frontend, driver_kwargs=VIDEO_KW, workers=4, depth=1)
    files = _check_expression_tree(out, jobs, hand_video, source=again)
    assert (res["videos"], res["frames"], res["files"]) == (5, 22, files)
    _afterwards(base)
