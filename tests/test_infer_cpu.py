"""No GPU: the split driver's host side (tce_rvos_amd.infer) -- jobs from a meta file, the frame prefetcher (what it yields, how
far it reads ahead, how its errors and its threads end) and run_split through its run= / encode= seams with Pillow as the encoder."""
import io
import json
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from tce_rvos_amd import infer
from tce_rvos_amd.dist import shard_range

H, W = 24, 40
LENGTHS = {"a": 3, "b": 1, "c": 5}
EXPRESSIONS = {"a": {"0": "a dog", "1": "the dog that runs to the left"},
               "b": {"3": "a person"},
               "c": {"1": "a red car", "0": "the car", "2": "the car which is parked behind the tree"}}  # key order, not sorted
PALETTE = bytes((37 * k + 11 * c) % 256 for k in range(256) for c in range(3))


def _image(seed, h=H, w=W):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 6 + seed * 31) % 256, (y * 9 + seed * 17) % 256, ((x + y) * 4) % 256], -1)
    return np.clip(base + rng.integers(-20, 20, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.fixture()
def split(tmp_path):
    """videos of 3, 1 and 5 frames of 24 x 40; video a holds a greyscale JPEG, video c a palette PNG"""
    jobs, seed = [], 0
    for name, n in LENGTHS.items():
        d = tmp_path / "frames" / name
        d.mkdir(parents=True)
        paths, names = [], []
        for k in range(n):
            seed += 1
            im = Image.fromarray(_image(seed))
            fname = "%05d" % (5 * k)
            if name == "a" and k == 1:
                im, p = im.convert("L"), d / (fname + ".jpg")
            elif name == "c" and k == 2:
                im, p = im.quantize(16), d / (fname + ".png")
            else:
                p = d / (fname + ".jpg")
            im.save(p, quality=90)
            paths.append(str(p))
            names.append(fname)
        jobs.append(infer.VideoJob(name, paths, names, dict(EXPRESSIONS[name])))
    assert Image.open(jobs[0].frame_paths[1]).mode == "L" and Image.open(jobs[2].frame_paths[2]).mode == "P"
    return jobs


def _want(job):
    return np.stack([np.asarray(Image.open(p).convert("RGB")) for p in job.frame_paths])


def _begun(timeline):
    return {v for s, v, e, _ in timeline if s == "decode" and e == "begin"}


# ---------------------------------------------------------------------------------------------------------------- the prefetcher
@pytest.mark.parametrize("workers", [1, 4])
def test_prefetcher_yields_pillow_s_frames_in_job_order(split, workers):
    base = threading.active_count()
    seen = []
    with infer.FramePrefetcher(split, workers=workers, depth=2, pin=False) as pf:
        assert len(pf) == 3
        for job, frames in pf:
            assert isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and not frames.is_cuda
            want = _want(job)
            assert tuple(frames.shape) == want.shape == (LENGTHS[job.name], H, W, 3)
            assert np.array_equal(frames.numpy(), want), job.name
            seen.append(job.name)
            pf.release(frames)
    assert seen == ["a", "b", "c"]
    assert threading.active_count() == base


def test_a_tensor_that_was_not_released_is_not_written_under_its_holder(split):
    with infer.FramePrefetcher(split, workers=2, depth=2, pin=False) as pf:
        _, first = next(pf)
        keep = first.clone()
        job, second = next(pf)  # releases `first` for its holder
        assert np.array_equal(second.numpy(), _want(job))
        assert first.data_ptr() != second.data_ptr()
        _, third = next(pf)
        assert third.data_ptr() != second.data_ptr()
        pf.release(third)
        pf.release(third)  # idempotent
    del keep


@pytest.mark.parametrize("depth", [0, 1])
def test_decoding_stops_depth_videos_ahead_of_the_consumer(split, depth, monkeypatch):
    base = threading.active_count()
    decoded, real = [], infer._decode

    def hook(path):
        decoded.append(os.path.basename(os.path.dirname(path)))
        return real(path)

    monkeypatch.setattr(infer, "_decode", hook)
    pf = infer.FramePrefetcher(split, workers=4, depth=depth, pin=False)
    try:
        assert _begun(pf.timeline) == set(range(depth + 1))  # construction submits depth + 1 videos at once
        next(pf)
        assert _begun(pf.timeline) == set(range(depth + 1))  # consuming video 0: videos 1 .. depth are ahead, no more
        next(pf)
        assert _begun(pf.timeline) == set(range(min(depth + 2, 3)))
    finally:
        pf.close()
    assert threading.active_count() == base
    names = ["a", "b", "c"]
    assert set(decoded) <= set(names[:depth + 2]) and {"a", "b"} <= set(decoded)
    assert decoded.count("a") == 3 and decoded.count("b") == 1


def test_a_truncated_jpeg_raises_at_its_video_with_its_path(split, tmp_path):
    base = threading.active_count()
    bad = tmp_path / "frames" / "b" / "cut.jpg"
    data = open(split[1].frame_paths[0], "rb").read()
    bad.write_bytes(data[:len(data) // 2])
    split[1] = infer.VideoJob("b", [str(bad)], ["00000"], split[1].expressions)
    pf = infer.FramePrefetcher(split, workers=4, depth=2, pin=False)
    job, frames = next(pf)
    assert job.name == "a" and np.array_equal(frames.numpy(), _want(job))
    with pytest.raises(infer.DecodeError) as e:
        next(pf)
    assert str(bad) in str(e.value)
    assert threading.active_count() == base  # the error closed the prefetcher
    with pytest.raises(StopIteration):
        next(pf)


def test_a_missing_file_raises_at_its_video_with_its_path(split):
    base = threading.active_count()
    gone = split[2].frame_paths[3] + ".nothing"
    split[2].frame_paths[3] = gone
    with infer.FramePrefetcher(split, workers=2, depth=0, pin=False) as pf:
        next(pf)
        next(pf)
        with pytest.raises(infer.DecodeError) as e:
            next(pf)
        assert gone in str(e.value)
    assert threading.active_count() == base


def test_frames_of_two_sizes_in_one_video_are_a_value_error(split, tmp_path):
    base = threading.active_count()
    odd = tmp_path / "frames" / "c" / "odd.jpg"
    Image.fromarray(_image(99, H - 4, W)).save(odd)
    split[2].frame_paths[4] = str(odd)
    with infer.FramePrefetcher(split[2:], workers=4, depth=2, pin=False) as pf:
        with pytest.raises(ValueError) as e:
            next(pf)
        assert str(odd) in str(e.value) and not isinstance(e.value, infer.DecodeError)
    assert threading.active_count() == base


@pytest.mark.parametrize("workers", [0, 17, -1, 2.0, True])
def test_workers_outside_1_to_16_are_refused(split, workers):
    base = threading.active_count()
    with pytest.raises(ValueError):
        infer.FramePrefetcher(split, workers=workers, pin=False)
    with pytest.raises(ValueError):
        infer.run_split(None, split, "unused", workers=workers, frontend=lambda x: x, run=_fake_run, encode=_encode_l)
    assert threading.active_count() == base


def test_the_default_worker_count_is_the_constant_8():
    import inspect
    assert inspect.signature(infer.FramePrefetcher).parameters["workers"].default == 8
    assert inspect.signature(infer.run_split).parameters["workers"].default == 8
    src = inspect.getsource(infer)
    assert "cpu_count" not in src and "multiprocessing" not in src and "subprocess" not in src


def test_close_in_the_middle_joins_every_thread(split):
    base = threading.active_count()
    pf = infer.FramePrefetcher(split, workers=4, depth=2, pin=False)
    next(pf)
    pf.close()
    pf.close()
    assert threading.active_count() == base
    with pytest.raises(StopIteration):
        next(pf)
    with pytest.raises(RuntimeError, match="consumer"):
        with infer.FramePrefetcher(split, workers=4, depth=2, pin=False) as pf:
            next(pf)
            raise RuntimeError("the consumer failed")
    assert threading.active_count() == base


# --------------------------------------------------------------------------------------------------------------- jobs_from_meta
def test_jobs_from_meta(tmp_path):
    videos = {"zebra": {"frames": ["00000", "00005"], "expressions": {"1": {"exp": "The  Zebra "}, "0": {"exp": "a zebra"}}},
              "ant": {"frames": ["00010"], "expressions": {"10": {"exp": "an ant"}, "2": {"exp": "ant two"}, "3": {"exp": "x"}}}}
    jobs = infer.jobs_from_meta(videos, "imgs")
    assert [j.name for j in jobs] == ["ant", "zebra"]
    assert list(jobs[0].expressions.items()) == [("10", "an ant"), ("2", "ant two"), ("3", "x")]
    assert list(jobs[1].expressions.items()) == [("1", "The  Zebra "), ("0", "a zebra")]  # key order, text untouched
    assert list(jobs[1].frame_names) == ["00000", "00005"]
    assert list(jobs[1].frame_paths) == [os.path.join("imgs", "zebra", "00000.jpg"), os.path.join("imgs", "zebra", "00005.jpg")]
    meta = tmp_path / "meta_expressions.json"
    meta.write_text(json.dumps({"videos": videos}))
    assert infer.jobs_from_meta(str(meta), "imgs") == jobs and infer.jobs_from_meta(meta, "imgs") == jobs
    assert list(infer.jobs_from_meta(videos, "x", ext=".png")[0].frame_paths) == [os.path.join("x", "ant", "00010.png")]


# -------------------------------------------------------------------------------------------------------------------- run_split
def _fake_run(model, frames, job, origin_hw):
    assert model is None and tuple(frames.shape[1:3]) == tuple(origin_hw) == (H, W)
    return [{"masks": (frames[..., 0] > 60 * (i + 1)).to(torch.uint8)} for i in range(len(job.expressions))]


def _fake_run_objects(model, frames, job, origin_hw):
    return [{"labels": (frames[..., 0].to(torch.int32) * (k + 2) // 128).to(torch.uint8)} for k in range(2)]


def _png(im):
    buf = io.BytesIO()
    im.save(buf, format="PNG")
    return buf.getvalue()


def _encode_l(planes):
    return [_png(Image.fromarray(p.numpy() * 255, "L")) for p in planes]


def _encode_p(planes):
    out = []
    for p in planes:
        im = Image.fromarray(p.numpy(), "P")
        im.putpalette(PALETTE)
        out.append(_png(im))
    return out


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs}


def _check_video_tree(out, jobs):
    want = {os.path.join(j.name, e, f + ".png") for j in jobs for e in j.expressions for f in j.frame_names}
    assert _tree(out) == want
    for j in jobs:
        red = _want(j)[..., 0]
        for i, e in enumerate(j.expressions):
            for k, f in enumerate(j.frame_names):
                im = Image.open(os.path.join(out, j.name, e, f + ".png"))
                assert im.mode == "L" and np.array_equal(np.asarray(im), (red[k] > 60 * (i + 1)).astype(np.uint8) * 255), (j.name, e, f)
    return want


def _check_result(res, jobs, files, depth):
    assert res["videos"] == len(jobs) and res["frames"] == sum(len(j.frame_paths) for j in jobs)
    assert res["pairs"] == sum(len(j.expressions) for j in jobs) and res["files"] == files
    assert set(res["busy"]) == set(infer.STAGES) and all(v >= 0 for v in res["busy"].values())
    assert res["seconds"] > 0
    tl = res["timeline"]
    assert [t for *_, t in tl] == sorted(t for *_, t in tl)
    for stage in infer.STAGES:
        for v in range(len(jobs)):
            at = [k for k, (s, i, _, _) in enumerate(tl) if s == stage and i == v]
            assert [tl[k][2] for k in at] == ["begin", "end"], (stage, v)
    # submission order: videos 0 .. depth are handed to the decoders before the first forward begins
    first_forward = tl.index(next(ev for ev in tl if ev[:3] == ("forward", 0, "begin")))
    for v in range(min(depth + 1, len(jobs))):
        assert tl.index(next(ev for ev in tl if ev[:3] == ("decode", v, "begin"))) < first_forward, v


@pytest.mark.parametrize("workers,depth,writers", [(4, 2, 2), (1, 0, 1), (8, 1, 3)])
def test_run_split_writes_the_expression_tree(split, tmp_path, workers, depth, writers):
    base = threading.active_count()
    out = str(tmp_path / "out")
    res = infer.run_split(None, split, out, mode="video", frontend=lambda x: x, run=_fake_run, encode=_encode_l, workers=workers,
                          depth=depth, writers=writers)
    want = _check_video_tree(out, split)
    _check_result(res, split, len(want), depth)
    assert threading.active_count() == base


def test_run_split_writes_the_annotator_tree(split, tmp_path):
    base = threading.active_count()
    out = str(tmp_path / "out")
    res = infer.run_split(None, split, out, mode="objects", palette=PALETTE, frontend=lambda x: x, run=_fake_run_objects,
                          encode=_encode_p)
    want = {os.path.join(f"anno_{k}", j.name, "%05d.png" % f) for k in range(2) for j in split for f in range(len(j.frame_paths))}
    assert _tree(out) == want
    for j in split:
        red = _want(j)[..., 0].astype(np.int32)
        for k in range(2):
            for f in range(len(j.frame_paths)):
                im = Image.open(os.path.join(out, f"anno_{k}", j.name, "%05d.png" % f))
                assert im.mode == "P" and bytes(im.getpalette()) == PALETTE
                assert np.array_equal(np.asarray(im), (red[f] * (k + 2) // 128).astype(np.uint8)), (j.name, k, f)
    _check_result(res, split, len(want), 2)
    assert threading.active_count() == base


def test_a_rank_runs_its_own_block(split, tmp_path):
    out = str(tmp_path / "out")
    lo, hi = shard_range(len(split), 1, 2)
    assert 0 < lo < hi == 3
    res = infer.run_split(None, split, out, frontend=lambda x: x, run=_fake_run, encode=_encode_l, rank=1, world=2)
    want = _check_video_tree(out, split[lo:hi])
    _check_result(res, split[lo:hi], len(want), 2)
    out0 = str(tmp_path / "out0")
    res0 = infer.run_split(None, split, out0, frontend=lambda x: x, run=_fake_run, encode=_encode_l, rank=0, world=2)
    _check_video_tree(out0, split[:lo])
    assert res0["videos"] + res["videos"] == len(split)
    empty = infer.run_split(None, split[:1], str(tmp_path / "none"), frontend=lambda x: x, run=_fake_run, encode=_encode_l,
                            rank=1, world=2)
    assert empty["videos"] == empty["files"] == 0 and empty["timeline"] == []


def test_a_writer_s_failure_is_raised_after_every_thread_has_joined(split, tmp_path):
    base = threading.active_count()
    out = tmp_path / "out"
    out.mkdir()
    (out / "b").write_bytes(b"a file where video b's directory has to be")
    with pytest.raises(OSError) as e:
        infer.run_split(None, split, str(out), frontend=lambda x: x, run=_fake_run, encode=_encode_l, writers=2)
    assert str(out / "b") in str(e.value)
    assert threading.active_count() == base
    assert os.path.isfile(out / "b")


def test_a_failure_in_the_driver_joins_every_thread(split, tmp_path):
    base = threading.active_count()

    def run(model, frames, job, origin_hw):
        if job.name == "b":
            raise RuntimeError("the driver failed")
        return _fake_run(model, frames, job, origin_hw)

    with pytest.raises(RuntimeError, match="the driver failed"):
        infer.run_split(None, split, str(tmp_path / "out"), frontend=lambda x: x, run=run, encode=_encode_l)
    assert threading.active_count() == base


def test_objects_without_a_palette_and_unknown_modes_fail_before_any_decode(split, tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(infer, "_decode", lambda path: calls.append(path))
    monkeypatch.setattr(infer, "FramePrefetcher", lambda *a, **k: calls.append("prefetcher"))
    with pytest.raises(ValueError, match="palette"):
        infer.run_split(None, split, str(tmp_path / "out"), mode="objects", frontend=lambda x: x, run=_fake_run_objects,
                        encode=_encode_p)
    with pytest.raises(ValueError, match="mode"):
        infer.run_split(None, split, str(tmp_path / "out"), mode="clips", frontend=lambda x: x, run=_fake_run, encode=_encode_l)
    with pytest.raises(ValueError, match="writers"):
        infer.run_split(None, split, str(tmp_path / "out"), writers=0, frontend=lambda x: x, run=_fake_run, encode=_encode_l)
    assert calls == [] and not os.path.exists(tmp_path / "out")
