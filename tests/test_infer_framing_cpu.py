"""CPU: run_split's framing= argument with stand-ins for the front-end, the driver and the encoder (the way tests/test_infer_cpu.py
drives it): both values are accepted and a caller's encoder is untouched by them; any other value is refused before a frame is
decoded."""
import io
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from tce_rvos_amd import infer

H, W = 12, 20


@pytest.fixture()
def split(tmp_path):
    jobs = []
    for v, (name, n) in enumerate((("a", 2), ("b", 3))):
        d = tmp_path / "frames" / name
        d.mkdir(parents=True)
        paths, names = [], []
        for k in range(n):
            y, x = np.mgrid[0:H, 0:W]
            img = np.stack([(x * 12 + 40 * k + 7 * v) % 256, (y * 20) % 256, (x + y) % 256], -1).astype(np.uint8)
            p = d / ("%05d.png" % k)
            Image.fromarray(img).save(p)
            paths.append(str(p))
            names.append("%05d" % k)
        jobs.append(infer.VideoJob(name, paths, names, {"0": "a dog", "1": "the dog"}))
    return jobs


def _run(model, frames, job, origin_hw):
    return [{"masks": (frames[..., 0] > 90 * (i + 1)).to(torch.uint8)} for i in range(len(job.expressions))]


def _encode(planes):
    out = []
    for p in planes:
        buf = io.BytesIO()
        Image.fromarray(p.numpy() * 255, "L").save(buf, format="PNG")
        out.append(buf.getvalue())
    return out


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_both_framings_are_accepted_and_leave_a_callers_encoder_alone(split, tmp_path):
    base = threading.active_count()
    trees = []
    for framing in ("host", "device", None):
        out = str(tmp_path / f"out_{framing}")
        kw = {} if framing is None else {"framing": framing}
        res = infer.run_split(None, split, out, frontend=lambda x: x, run=_run, encode=_encode, **kw)
        assert res["videos"] == 2 and res["files"] == 2 * (2 + 3)
        trees.append(_tree(out))
    assert trees[0] == trees[1] == trees[2] and len(trees[0]) == 10  # the same files, byte for byte: encode= is the caller's
    assert threading.active_count() == base


@pytest.mark.parametrize("bad", ["gpu", "Device", "", None, 1])
def test_an_unknown_framing_fails_before_any_decode(split, tmp_path, bad, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a prefetcher was built")
    monkeypatch.setattr(infer, "FramePrefetcher", boom)
    with pytest.raises(ValueError, match="framing"):
        infer.run_split(None, split, str(tmp_path / "out"), frontend=lambda x: x, run=_run, encode=_encode, framing=bad)
    assert not os.path.exists(tmp_path / "out")
