"""The split driver's overlays= (infer.run_split): without it nothing changes (no GPU: the run= / encode= seams of
tests/test_infer_cpu.py); with it, on the GPU, the overlay files are vis.overlay_expression / vis.overlay_objects + png.rgb_pngs
called by hand on the decoded frames, the mask files are the ones written without it, and device buffers that are reused hold the
right video when the overlay launches read them."""
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from tce_rvos_amd import infer

H, W = 48, 64
COLORS = np.array([[236, 95, 17], [0, 114, 189], [119, 172, 48]], dtype=np.uint8)
EXPRESSIONS = {"kite": {"0": "a kite", "1": "the red kite"}, "boat": {"2": "a boat", "0": "the small boat", "1": "a white boat", "5": "it"}}


def _frame(seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 4 + seed * 31) % 256, (y * 5 + seed * 17) % 256, ((x + y) * 2) % 256], -1)
    return np.clip(base + rng.integers(-10, 10, (H, W, 3)), 0, 255).astype(np.uint8)


@pytest.fixture()
def split(tmp_path):
    """2 videos x 3 frames of 48 x 64"""
    jobs, seed = [], 0
    for name in ("kite", "boat"):
        d = tmp_path / "frames" / name
        d.mkdir(parents=True)
        names = ["%05d" % (5 * k) for k in range(3)]
        paths = [str(d / (f + ".jpg")) for f in names]
        for p in paths:
            seed += 1
            Image.fromarray(_frame(seed)).save(p, quality=90)
        jobs.append(infer.VideoJob(name, paths, names, dict(EXPRESSIONS[name])))
    return jobs


def _decoded(job):
    return np.stack([np.asarray(Image.open(p).convert("RGB")) for p in job.frame_paths])


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def _results(job, device):
    """a driver's dicts for `job`, made from its name alone: masks, boxes and points that differ per video, expression and frame"""
    n, key = len(job.frame_paths), sum(job.name.encode())
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(len(job.expressions)):
        masks = np.stack([((y - 20 - 3 * k - i) ** 2 + (x - 24 - 5 * i - key % 7) ** 2 < (9 + 2 * i) ** 2) for k in range(n)]).astype(np.uint8)
        boxes = np.array([[0.4 + 0.05 * i, 0.45 + 0.04 * k, 0.3 + 0.1 * i, 0.35 + (key % 5) * 0.02] for k in range(n)], np.float32)
        points = np.array([[0.2 + 0.15 * i, 0.1 + 0.3 * k] for k in range(n)], np.float32)
        out.append({"masks": torch.from_numpy(masks).to(device), "pred_boxes": torch.from_numpy(boxes).to(device),
                    "reference_points": torch.from_numpy(points).to(device)})
    return out


def _fake_run(model, frames, job, origin_hw):
    assert tuple(origin_hw) == (H, W)
    return _results(job, frames.device)


def _encode_l(planes):
    import io
    out = []
    for p in planes.cpu().numpy():
        buf = io.BytesIO()
        Image.fromarray(p * 255).save(buf, format="PNG")
        out.append(buf.getvalue())
    return out


# ----------------------------------------------------------------------------------------------------------------- no GPU
def test_without_overlays_the_files_and_the_timeline_are_todays(split, tmp_path):
    base = threading.active_count()
    a = infer.run_split(None, split, str(tmp_path / "a"), frontend=lambda x: x, run=_fake_run, encode=_encode_l, depth=1)
    b = infer.run_split(None, split, str(tmp_path / "b"), frontend=lambda x: x, run=_fake_run, encode=_encode_l, depth=1, overlays=None)
    ta, tb = _tree(str(tmp_path / "a")), _tree(str(tmp_path / "b"))
    assert ta == tb and len(ta) == 3 * 2 + 3 * 4
    assert set(ta) == {os.path.join(j.name, e, f + ".png") for j in split for e in j.expressions for f in j.frame_names}
    for res in (a, b):
        assert (res["videos"], res["frames"], res["pairs"], res["files"]) == (2, 6, 6, 18)
        assert set(res) == {"videos", "frames", "pairs", "files", "seconds", "busy", "timeline"}
        for stage in infer.STAGES:  # one begin and one end per stage and video, as before
            for v in range(2):
                assert [e for s, i, e, _ in res["timeline"] if s == stage and i == v] == ["begin", "end"], (stage, v)
    assert threading.active_count() == base


def test_overlays_need_the_device_path_and_a_well_formed_dict(split, tmp_path):
    base = threading.active_count()
    host = dict(frontend=lambda x: x, run=_fake_run, encode=_encode_l)
    with pytest.raises(ValueError, match="overlays"):
        infer.run_split(None, split, str(tmp_path / "a"), overlays={"dir": str(tmp_path / "o"), "colors": COLORS}, **host)
    for bad in ({"dir": "x"}, {"colors": COLORS}, {"dir": "x", "colors": COLORS.astype(np.int64)}, {"dir": "x", "colors": COLORS[:0]},
                {"dir": "x", "colors": COLORS.reshape(-1)}, {"dir": "x", "colors": COLORS, "colour": 1}, "x"):
        with pytest.raises(ValueError, match="overlays"):
            infer.run_split(None, split, str(tmp_path / "a"), overlays=bad, **host)
    assert not os.path.exists(tmp_path / "a") and not os.path.exists(tmp_path / "o")
    assert threading.active_count() == base


def test_overlay_items_name_the_reference_s_paths(split):
    job = split[1]
    res = [{"pred_boxes": torch.zeros(3, 4)} for _ in job.expressions]
    items = infer._overlay_items("video", "vis", job, res)
    assert [pos for _, _, pos in items] == [[0], [1], [2], [3]]                           # the position, not the expression id
    assert items[2][0] == [os.path.join("vis", "boat", "2", f + ".png") for f in job.frame_names]
    assert infer._overlay_items("windows", "vis", job, res)[0][0] == items[0][0]
    sets = [{"pred_boxes": torch.zeros(2, 3, 4)}, {"pred_boxes": torch.zeros(5, 3, 4)}]
    (paths, r, pos), = infer._overlay_items("objects", "vis", job, sets)
    assert r is sets[-1] and pos == [0, 1, 2, 3, 4] and paths == [os.path.join("vis", "boat", f + ".png") for f in job.frame_names]
    assert infer._overlay_items("objects", "vis", job, []) == []


# -------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 0])
def test_overlay_files_equal_the_hand_calls_and_the_mask_files_are_unchanged(split, tmp_path, depth):
    """five jobs over the two videos: each of the two device buffers is reused while the overlay launches of the video before it
    are the last readers of its frames"""
    from tce_rvos_amd import png, vis
    base = threading.active_count()
    jobs = list(split) + [infer.VideoJob(n, split[i].frame_paths, split[i].frame_names, split[i].expressions)
                          for n, i in (("kite2", 0), ("boat2", 1), ("kite3", 0))]
    plain = infer.run_split(None, jobs, str(tmp_path / "plain"), frontend=lambda x: x, run=_fake_run, depth=depth)
    res = infer.run_split(None, jobs, str(tmp_path / "out"), frontend=lambda x: x, run=_fake_run, depth=depth,
                          overlays={"dir": str(tmp_path / "vis"), "colors": COLORS})
    assert _tree(str(tmp_path / "out")) == _tree(str(tmp_path / "plain"))                  # the mask files: unchanged
    want = {}
    colors = torch.from_numpy(COLORS).cuda()
    for job in jobs:
        u8 = _decoded(job)
        frames = torch.from_numpy(u8).cuda()
        for i, r in enumerate(_results(job, frames.device)):
            img = vis.overlay_expression(frames, r, colors[i % 3])
            assert not np.array_equal(img.cpu().numpy(), u8)
            for f, blob in zip(job.frame_names, png.rgb_pngs(img)):
                want[os.path.join(job.name, str(i), f + ".png")] = blob
    got = _tree(str(tmp_path / "vis"))
    assert set(got) == set(want) and len(want) == 3 * (2 + 4 + 2 + 4 + 2)
    for k in want:
        assert got[k] == want[k], k
    im = Image.open(os.path.join(str(tmp_path / "vis"), "boat", "3", "00005.png"))
    assert im.mode == "RGB" and im.size == (W, H)
    assert res["files"] == plain["files"] + len(want) and res["videos"] == 5
    for stage in infer.STAGES:
        for v in range(5):
            assert [e for s, i, e, _ in res["timeline"] if s == stage and i == v] == ["begin", "end"], (stage, v)
    torch.cuda.synchronize()
    assert threading.active_count() == base


@pytest.mark.gpu
def test_objects_mode_draws_the_last_set_s_boxes(split, tmp_path):
    from tce_rvos_amd import png, vis
    palette = bytes(range(256)) * 3

    def sets_of(job, device):
        r = _results(job, device)
        boxes = torch.stack([x["pred_boxes"] for x in r])
        labels = torch.stack([x["masks"] for x in r]).amax(0)
        return [{"labels": labels, "pred_boxes": boxes[:1].contiguous()}, {"labels": labels, "pred_boxes": boxes.contiguous()}]

    run = lambda model, frames, job, hw: sets_of(job, frames.device)  # noqa: E731
    res = infer.run_split(None, split, str(tmp_path / "out"), mode="objects", palette=palette, frontend=lambda x: x, run=run,
                          overlays={"dir": str(tmp_path / "vis"), "colors": COLORS[:2]})
    got = _tree(str(tmp_path / "vis"))
    assert set(got) == {os.path.join(j.name, f + ".png") for j in split for f in j.frame_names}
    for job in split:
        frames = torch.from_numpy(_decoded(job)).cuda()
        boxes = sets_of(job, frames.device)[-1]["pred_boxes"]
        col = torch.from_numpy(COLORS[:2]).cuda()[[k % 2 for k in range(boxes.shape[0])]]
        for f, blob in zip(job.frame_names, png.rgb_pngs(vis.overlay_objects(frames, boxes, col))):
            assert got[os.path.join(job.name, f + ".png")] == blob, (job.name, f)
    assert res["files"] == 2 * 2 * 3 + 2 * 3
