"""A dataset split, end to end: the loop of the reference's inference drivers (inference_ytvos.py:166-363, inference_davis.py:
150-311, inference_mevis.py:160-214) with the host stages beside the forward instead of in front of it.

    jobs = jobs_from_meta("meta_expressions.json", "JPEGImages")
    run_split(model, jobs, "out", driver_kwargs={"clip_size": None})

* A video is decoded ONCE, whatever the number of its expressions (the reference decodes it again for every expression), by a pool
  of host threads that runs `depth` videos ahead of the forward (FramePrefetcher: Pillow releases the GIL while it decodes).
* The decoded frames go to the device on a side stream while the video before them is still in its forward.
* The forward is the existing driver, called unchanged, once per video with all of its captions (video.run_video_expressions /
  run_video_windows / run_video_objects): every mask is what a sequential loop over the same calls produces, bit for bit.
* The PNG streams are made on the device (png.mask_pngs / label_pngs); writer threads create the directories and write the files
  while the next video runs.
* overlays= additionally writes the drivers' --visualize images (vis.overlay_expression / overlay_objects on the raw frames that
  are on the device already, png.rgb_pngs), through the same writer threads.

No kernel is added here: the module is host orchestration over launches that exist.  Threads only, never processes; no pool size
is read from the machine.
"""
import json
import os
import queue
import threading
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Mapping, Sequence

import numpy as np
import torch
from PIL import Image

from . import dist, png, video, vis

MAX_WORKERS = 16
STAGES = ("decode", "upload_wait", "forward", "encode", "write")
MODES = ("video", "windows", "objects")


class DecodeError(RuntimeError):
    """A frame that Pillow could not open or decode; the message starts with the file's path."""


@dataclass
class VideoJob:
    """One video of a split.  frame_paths[k] is the file of frame frame_names[k]; expressions: ordered mapping exp_id -> text."""
    name: str
    frame_paths: Sequence[str]
    frame_names: Sequence[str]
    expressions: Mapping[str, str]


def jobs_from_meta(meta, img_folder, ext=".jpg"):
    """The jobs of a `meta_expressions.json` (Ref-YouTube-VOS, MeViS, the converted Ref-DAVIS): meta is the file's path or its
    loaded ["videos"] dict, videos[video]["frames"] the frame names and videos[video]["expressions"][id]["exp"] the captions.
    Videos in sorted order, expressions in the order of the mapping's keys (inference_ytvos.py:85,170-182), frame k of a video at
    img_folder/<video>/<frame><ext>.  Captions are passed on exactly as the file holds them."""
    if isinstance(meta, (str, bytes, os.PathLike)):
        with open(meta) as f:
            meta = json.load(f)["videos"]
    jobs = []
    for name in sorted(meta):
        frames = [str(f) for f in meta[name]["frames"]]
        exps = meta[name]["expressions"]
        jobs.append(VideoJob(name, [os.path.join(str(img_folder), name, f + ext) for f in frames], frames,
                             {k: exps[k]["exp"] for k in exps.keys()}))
    return jobs


def _decode(path):
    """The decode rule of every frame, the reference's own (inference_ytvos.py:283): uint8 [H,W,3]"""
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


class _Timeline:
    """(stage, video, "begin"|"end", t) in the order the events happened, from whichever thread"""

    def __init__(self):
        self.events = []
        self.busy = {s: 0.0 for s in STAGES}
        self._lock = threading.Lock()

    def mark(self, stage, v, edge):
        with self._lock:
            t = time.perf_counter()
            self.events.append((stage, v, edge, t))
        return t

    def add(self, stage, seconds):
        with self._lock:
            self.busy[stage] += seconds


class _Pending:
    """a video between its submission and its release"""

    def __init__(self, index, job):
        self.index, self.job = index, job
        self.flat = self.tensor = self.array = None
        self.left, self.error = 0, None
        self.lock, self.done = threading.Lock(), threading.Event()


class FramePrefetcher:
    """Iterator and context manager over `jobs`: yields (job, frames_u8) in job order, frames_u8 a uint8 [N,H,W,3] host tensor
    whose frame k is np.asarray(Image.open(job.frame_paths[k]).convert("RGB")).

    A pool of `workers` threads (1 .. 16; threads, because Pillow decodes outside the GIL) decodes every frame straight into the
    video's staging buffer.  Construction submits videos 0 .. depth; the next() that hands out video k submits video k + depth, so
    at most `depth` videos are decoded ahead of the one being consumed and at most depth + 1 staging buffers exist.  A staging
    buffer goes back to the pool when its consumer released it -- release(frames_u8), or the next next() -- and not before: the
    tensor a consumer holds is never written under it.  The buffers are pinned when `pin` is true (default: where there is a GPU);
    they are allocated on the consumer's thread, the workers call nothing but Pillow and numpy.

    Frames of one video must have one size (ValueError, naming the file); a frame that does not decode is a DecodeError with its
    path.  Either reaches the consumer at the next() of its video.  close(), __exit__, the end of the iteration and an error
    handed to the consumer all stop and join the threads."""

    def __init__(self, jobs, workers=8, depth=2, pin=None):
        if isinstance(workers, bool) or not isinstance(workers, int) or not 1 <= workers <= MAX_WORKERS:
            raise ValueError(f"FramePrefetcher: workers must be an int in 1..{MAX_WORKERS}, got {workers!r}")
        if isinstance(depth, bool) or not isinstance(depth, int) or depth < 0:
            raise ValueError(f"FramePrefetcher: depth must be an int >= 0, got {depth!r}")
        self.jobs = list(jobs)
        self.workers, self.depth = workers, depth
        self.pin = torch.cuda.is_available() if pin is None else bool(pin)
        self._tl = _Timeline()
        self._pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="tce-decode")
        self._free = []           # staging buffers (flat uint8) nobody holds
        self._live = {}           # data_ptr of a yielded tensor -> its _Pending
        self._inflight = deque()  # submitted, not yet yielded
        self._submitted = 0
        self._closed = False
        try:
            while self._submitted < min(depth + 1, len(self.jobs)):
                self._submit()
        except BaseException:
            self.close()
            raise

    @property
    def timeline(self):
        return self._tl.events

    @property
    def decode_seconds(self):
        return self._tl.busy["decode"]

    def __len__(self):
        return len(self.jobs)

    def __iter__(self):
        return self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _take(self, nbytes):
        """a staging buffer of at least nbytes.  A video alive (submitted, not released) holds one buffer and a free one is
        dropped before a new one is made, so the buffers never outnumber the videos alive: depth + 1."""
        fit = [b for b in self._free if b.numel() >= nbytes]
        if fit:
            buf = min(fit, key=lambda b: b.numel())
            self._free = [b for b in self._free if b is not buf]
            return buf
        if self._free:
            self._free.remove(min(self._free, key=lambda b: b.numel()))
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=self.pin)

    def _submit(self):
        v = self._submitted
        p = _Pending(v, self.jobs[v])
        self._submitted += 1
        self._inflight.append(p)
        self._tl.mark("decode", v, "begin")
        paths = list(p.job.frame_paths)
        try:
            if not paths:
                raise ValueError(f"FramePrefetcher: video {p.job.name!r} has no frames")
            try:
                with Image.open(paths[0]) as im:  # the header only: the video's size, before any frame is decoded
                    w, h = im.size
            except Exception as e:
                raise DecodeError(f"{paths[0]}: {e}") from e
            need = len(paths) * h * w * 3
            p.flat = self._take(need)
            p.tensor = p.flat[:need].view(len(paths), h, w, 3)
            p.array = p.tensor.numpy()
        except Exception as e:
            p.error = e
            self._tl.mark("decode", v, "end")
            p.done.set()
            return
        p.left = len(paths)
        for k, path in enumerate(paths):
            self._pool.submit(self._frame, p, k, path)

    def _frame(self, p, k, path):
        err, t0 = None, time.perf_counter()
        try:
            if not self._closed and p.error is None:
                try:
                    a = _decode(path)
                except Exception as e:
                    raise DecodeError(f"{path}: {e}") from e
                if a.shape != p.array.shape[1:]:
                    raise ValueError(f"{path}: frame of {a.shape[1]} x {a.shape[0]} in a video of {p.array.shape[2]} x "
                                     f"{p.array.shape[1]} ({p.job.frame_paths[0]})")
                np.copyto(p.array[k], a)
        except Exception as e:
            err = e
        self._tl.add("decode", time.perf_counter() - t0)
        with p.lock:
            if err is not None and p.error is None:
                p.error = err
            p.left -= 1
            last = p.left == 0
        if last:
            self._tl.mark("decode", p.index, "end")
            p.done.set()

    def ready(self):
        """True when the next next() would not wait for a decode"""
        return bool(self._inflight) and self._inflight[0].done.is_set()

    def release(self, frames_u8):
        """The consumer is done with a yielded tensor: its staging buffer may be decoded into again.  (Idempotent.)"""
        p = self._live.pop(frames_u8.data_ptr(), None)
        if p is not None and p.flat is not None:
            self._free.append(p.flat)
            p.flat = p.tensor = p.array = None

    def __next__(self):
        if self._closed:
            raise StopIteration
        for p in list(self._live.values()):  # a consumer that never called release()
            self.release(p.tensor)
        if not self._inflight and self._submitted == len(self.jobs):
            self.close()
            raise StopIteration
        try:
            if not self._inflight:  # depth = 0: nothing is decoded ahead
                self._submit()
            p = self._inflight.popleft()
            while self._submitted < min(p.index + self.depth + 1, len(self.jobs)):
                self._submit()
            p.done.wait()
        except BaseException:
            self.close()
            raise
        if p.error is not None:
            self.close()
            raise p.error
        self._live[p.tensor.data_ptr()] = p
        return p.job, p.tensor

    def close(self):
        """Stops the decoding (frames not begun are dropped) and joins every thread."""
        self._closed = True
        self._pool.shutdown(wait=True, cancel_futures=True)
        self._inflight.clear()
        self._live.clear()
        self._free = []


class _Writers:
    """`n` threads behind a queue of at most 2 * n videos: each item is one video's (paths, blobs); the thread creates the
    directories and calls png.write_files.  The first exception is kept (later items are taken off the queue and dropped, so the
    producer never blocks on a dead consumer) and handed to run_split after close() has joined the threads."""

    def __init__(self, n, timeline):
        self.error = None
        self._tl = timeline
        self._lock = threading.Lock()
        self._q = queue.Queue(maxsize=2 * n)  # bounded: blobs cannot pile up behind a slow disk
        self._threads = [threading.Thread(target=self._loop, name=f"tce-write-{k}", daemon=True) for k in range(n)]
        for t in self._threads:
            t.start()

    def _loop(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            if self.error is not None:
                continue
            v, paths, blobs = item
            t0 = self._tl.mark("write", v, "begin")
            try:
                for d in dict.fromkeys(os.path.dirname(p) for p in paths):
                    os.makedirs(d, exist_ok=True)
                png.write_files(paths, blobs)
            except BaseException as e:
                with self._lock:
                    if self.error is None:
                        self.error = e
            self._tl.add("write", self._tl.mark("write", v, "end") - t0)

    def put(self, v, paths, blobs):
        self._q.put((v, paths, blobs))

    def close(self):
        for _ in self._threads:
            self._q.put(None)
        for t in self._threads:
            t.join()


class _Uploader:
    """Two raw-frame buffers on the device, filled alternately on a side stream.

    Ordering invariant 1: a device input buffer is not overwritten by a later upload before the front-end kernels that read it
    have finished.  `free[k]` is an event recorded on the compute stream after the last front-end call that read buffer k (for a
    buffer just allocated: at its allocation, since the allocator may hand out a block that earlier compute-stream work still
    uses); the side stream waits for it before the copy into buffer k.  The buffers are allocated and dropped with the compute
    stream current, so a dropped one is reused in that stream's order, behind its last reader."""

    def __init__(self, device):
        self.device = device
        self.compute = torch.cuda.current_stream(device)
        self.side = torch.cuda.Stream(device=device)
        self.bufs, self.free = [None, None], [None, None]

    def upload(self, v, host):
        """host [N,H,W,3] uint8 (pinned: the copy does not block) -> (its device copy, the copy's event on the side stream)"""
        k, need = v % 2, host.numel()
        if self.bufs[k] is None or self.bufs[k].numel() < need:
            self.bufs[k] = None
            self.bufs[k] = torch.empty(need, dtype=torch.uint8, device=self.device)
            self.free[k] = torch.cuda.Event()
            self.free[k].record(self.compute)
        dev = self.bufs[k][:need].view(host.shape)
        self.side.wait_event(self.free[k])  # invariant 1
        with torch.cuda.stream(self.side):
            dev.copy_(host, non_blocking=True)
        copied = torch.cuda.Event()
        copied.record(self.side)
        return dev, copied

    def consumed(self, v):
        """every call that reads buffer v % 2 -- the front-end, and with overlays on the video's overlay launches -- has been issued
        on the compute stream"""
        self.free[v % 2] = torch.cuda.Event()
        self.free[v % 2].record(self.compute)


def _default_run(mode, kw, ref_points=False):
    def run(model, frames, job, origin_hw):
        captions = list(job.expressions.values())
        if mode == "video":  # (ref_points: the overlays' cross; the windows driver returns the points anyway)
            return video.run_video_expressions(model, frames, captions, origin_hw, **({"ref_points": True, **kw} if ref_points else kw))
        if mode == "windows":
            return video.run_video_windows(model, frames, captions, origin_hw, **kw)
        k = dict(kw)
        if callable(k.get("object_sets")):  # e.g. video.davis_annotator_sets: the sets depend on the video's expression count
            k["object_sets"] = k["object_sets"](len(captions))
        return video.run_video_objects(model, frames, captions, origin_hw, **k)
    return run


def _paths(mode, out_dir, job, n_results, n_frames):
    """one list of paths per result of `run`, in order"""
    if mode == "objects":  # inference_davis.py:305-311
        return [[os.path.join(out_dir, f"anno_{k}", job.name, "%05d.png" % f) for f in range(n_frames)] for k in range(n_results)]
    exp_ids = list(job.expressions.keys())
    if n_results != len(exp_ids):
        raise ValueError(f"run_split: {n_results} results for the {len(exp_ids)} expressions of video {job.name!r}")
    return [[os.path.join(out_dir, job.name, str(e), str(f) + ".png") for f in job.frame_names] for e in exp_ids]  # inference_ytvos.py:355-363


def _check_overlays(overlays):
    """overlays= of run_split -> (dir, colors uint8 [K,3] on the host, rows_per_strip or None)"""
    if not isinstance(overlays, Mapping) or "dir" not in overlays or "colors" not in overlays or set(overlays) - {"dir", "colors", "rows_per_strip"}:
        raise ValueError("run_split: overlays must be dict(dir=..., colors=uint8 [K,3]) (optionally rows_per_strip=)")
    colors = torch.as_tensor(overlays["colors"])
    if colors.dtype != torch.uint8 or colors.dim() != 2 or colors.shape[0] < 1 or colors.shape[1] != 3:
        raise ValueError(f"run_split: overlays['colors'] must be uint8 [K,3] with K >= 1, got {colors.dtype} {list(colors.shape)}")
    return os.fspath(overlays["dir"]), colors.cpu().contiguous(), overlays.get("rows_per_strip")


def _overlay_items(mode, ov_dir, job, results):
    """What the overlay files of one video are made from, in order: (paths, result, colour positions).  Modes "video" and "windows":
    one image series per expression, <dir>/<video>/<expression position>/<frame_name>.png, colour `position` (inference_ytvos.py:
    337-350).  Mode "objects": the boxes of ONE object set's objects, colour `object`, at <dir>/<video>/<frame_name>.png -- the
    reference writes every annotator's image to that one path (inference_davis.py:287-291), so the last set's is what it leaves, and
    only that one is made here."""
    if mode == "objects":
        if not results:
            return []
        r = results[-1]
        return [([os.path.join(ov_dir, job.name, str(f) + ".png") for f in job.frame_names], r, list(range(int(r["pred_boxes"].shape[0]))))]
    return [([os.path.join(ov_dir, job.name, str(i), str(f) + ".png") for f in job.frame_names], r, [i]) for i, r in enumerate(results)]


def run_split(model, jobs, out_dir, *, mode="video", frontend=None, driver_kwargs=None, palette=None, codes="fixed",
              rows_per_strip=None, workers=8, depth=2, writers=2, rank=0, world=1, run=None, encode=None, overlays=None,
              framing="host"):
    """Every video of `jobs` (this rank's block of them: dist.shard_range(len(jobs), rank, world); no collective, each process
    writes its own files) through decode, upload, front-end, driver, PNG encoder and file writer.

    mode="video":   video.run_video_expressions(model, frames, captions, origin_hw, **driver_kwargs)  (clip_size=None: the
                    Ref-YouTube-VOS whole-video form) -> out_dir/<video>/<exp_id>/<frame_name>.png, mode L, 0 / 255 (png.mask_pngs)
    mode="windows": video.run_video_windows(...) (keep_fps / f_extra / MeViS), the same files
    mode="objects": video.run_video_objects(...) -> out_dir/anno_<k>/<video>/<%05d>.png, mode P with `palette` (png.label_pngs),
                    one k per object set; driver_kwargs["object_sets"] may be a function of the video's expression count
                    (video.davis_annotator_sets)
    frontend: decoded uint8 [N,H,W,3] on the device -> the model's clip; default frontend.ClipFrontEnd(), Resize(360).
    run(model, frames, job, origin_hw) -> list of dicts with "masks" ("labels" in objects mode) replaces the driver call,
    encode(planes) -> list of bytes replaces the PNG encoder.  With frontend, run and encode all given (and the front-end not a
    ClipFrontEnd) nothing here touches a GPU: no stream, no pinning, the frames stay host tensors.
    overlays=dict(dir=..., colors=uint8 [K,3]) (device path only) additionally writes the reference's --visualize images as RGB
    PNGs, drawn on the raw frames on the device (vis.overlay_expression / vis.overlay_objects, png.rgb_pngs).  "video" / "windows":
    <dir>/<video>/<expression position>/<frame_name>.png, one layer (mask tint, box, reference point -- the default driver is
    called with ref_points=True), colour colors[position % K].  "objects": <dir>/<video>/<frame_name>.png, the boxes of the last
    object set's objects, colour colors[object % K].  The files go through the same writer threads and count in `files`.  With
    overlays=None nothing changes.
    framing="host" | "device": where the PNG chunk framing and the IDAT's CRC-32 are made (png.encode); it goes to the default
    encoder and to the overlays' png.rgb_pngs, a caller's encode= is untouched.  The files are the same bytes either way.

    Returns dict(videos, frames, pairs (video x expression), files, seconds (wall), busy {decode, upload_wait, forward, encode,
    write: seconds summed over the stage's calls; decode over the worker threads' frames, write over the writer threads'
    videos; upload_wait is the time this thread waited for a decoded video and issued its copy}, timeline [(stage, video index in
    this rank's block, "begin"|"end", t)] in the order the events happened; a decode begins when it is submitted)."""
    if mode not in MODES:
        raise ValueError(f"run_split: mode must be one of {MODES}, got {mode!r}")
    if mode == "objects" and palette is None:
        raise ValueError("run_split: mode='objects' writes palette PNGs and needs `palette`")
    if isinstance(writers, bool) or not isinstance(writers, int) or not 1 <= writers <= MAX_WORKERS:
        raise ValueError(f"run_split: writers must be an int in 1..{MAX_WORKERS}, got {writers!r}")
    if framing not in png.FRAMINGS:
        raise ValueError(f"run_split: framing must be 'host' or 'device', got {framing!r}")
    jobs = list(jobs)
    lo, hi = dist.shard_range(len(jobs), int(rank), int(world))
    jobs = jobs[lo:hi]
    out_dir = os.fspath(out_dir)
    kw = dict(driver_kwargs or {})
    from .frontend import ClipFrontEnd
    on_device = frontend is None or run is None or encode is None or isinstance(frontend, ClipFrontEnd)
    if on_device and not torch.cuda.is_available():
        raise RuntimeError("run_split: the front-end, the driver and the PNG encoder run on the GPU and none is available "
                           "(there is no host fallback; pass frontend=, run= and encode= to drive the pipeline without one)")
    if frontend is None:
        frontend = ClipFrontEnd()
    ov = None if overlays is None else _check_overlays(overlays)
    if ov is not None and not on_device:
        raise ValueError("run_split: overlays are drawn and encoded on the GPU; they need the device path (frames on the device)")
    if run is None:
        run = _default_run(mode, kw, ref_points=ov is not None)
    if encode is None:
        if mode == "objects":
            encode = lambda planes: png.label_pngs(planes, palette, rows_per_strip=rows_per_strip, codes=codes, framing=framing)  # noqa: E731
        else:
            encode = lambda planes: png.mask_pngs(planes, rows_per_strip=rows_per_strip, codes=codes, framing=framing)  # noqa: E731
    key = "labels" if mode == "objects" else "masks"

    t_start = time.perf_counter()
    pf = FramePrefetcher(jobs, workers=workers, depth=depth, pin=on_device)
    tl = pf._tl
    up = _Uploader(torch.device("cuda", torch.cuda.current_device())) if on_device else None
    ov_colors = None if ov is None else ov[1].to(up.device)
    wr = _Writers(writers, tl)
    count = {"videos": 0, "frames": 0, "pairs": 0, "files": 0}

    def take(v, held):
        """Video v out of the prefetcher and on its way to the device: (job, host, dev, copied).
        Ordering invariant 2: a pinned staging buffer is not released before its copy's event has completed -- `held` is the
        video before, whose buffer this next() recycles, so its copy is waited for (on the host) first."""
        t0 = tl.mark("upload_wait", v, "begin")
        if held is not None:
            if held[3] is not None:
                held[3].synchronize()  # invariant 2
            pf.release(held[1])
        job, host = next(pf)
        dev, copied = up.upload(v, host) if on_device else (host, None)
        tl.add("upload_wait", tl.mark("upload_wait", v, "end") - t0)
        return job, host, dev, copied

    try:
        with pf:
            nxt = take(0, None) if jobs else None
            for v in range(len(jobs)):
                if wr.error is not None:
                    break
                cur, nxt = nxt, None
                job, host, dev, copied = cur
                # the video after this one goes up while this one computes, if it is decoded already (never wait for a decode
                # with the forward unissued).  On the host path `dev` IS the staging buffer: it is held until the encoder is done.
                if on_device and v + 1 < len(jobs) and pf.ready():
                    nxt = take(v + 1, cur)
                t0 = tl.mark("forward", v, "begin")
                if on_device:
                    up.compute.wait_event(copied)  # the front-end reads what the side stream wrote
                frames = frontend(dev)
                if on_device and ov is None:
                    up.consumed(v)  # invariant 1: recorded behind the front-end kernels, before anything else reads or waits
                origin_hw = (int(host.shape[1]), int(host.shape[2]))
                results = run(model, frames, job, origin_hw)
                tl.add("forward", tl.mark("forward", v, "end") - t0)
                t0 = tl.mark("encode", v, "begin")
                paths, blobs = [], []
                for ps, r in zip(_paths(mode, out_dir, job, len(results), int(host.shape[0])), results):
                    bs = list(encode(r[key]))
                    if len(bs) != len(ps):
                        raise ValueError(f"run_split: {len(bs)} files for the {len(ps)} frames of video {job.name!r}")
                    paths += ps
                    blobs += bs
                if ov is not None:
                    # Invariant 1 with overlays on: the overlay launches read the RAW frames `dev` long after the front-end did, so
                    # the buffer's `consumed` event is recorded behind the video's LAST overlay launch instead of behind the
                    # front-end -- the upload that overwrites this buffer (video v + 2, issued in a later iteration) waits for it
                    # on the side stream.  Every exit between here and that record ends the loop: no later upload is issued.
                    items = _overlay_items(mode, ov[0], job, results)
                    if not items:
                        up.consumed(v)
                    for k, (ps, r, pos) in enumerate(items):
                        col = ov_colors[[p % int(ov_colors.shape[0]) for p in pos]]
                        img = vis.overlay_objects(dev, r["pred_boxes"], col) if mode == "objects" else vis.overlay_expression(dev, r, col)
                        if k == len(items) - 1:
                            up.consumed(v)  # invariant 1 (above): behind the last launch that reads `dev`
                        bs = png.rgb_pngs(img, rows_per_strip=ov[2], framing=framing)
                        if len(bs) != len(ps):
                            raise ValueError(f"run_split: {len(bs)} overlay files for the {len(ps)} frames of video {job.name!r}")
                        paths += ps
                        blobs += bs
                        del img
                tl.add("encode", tl.mark("encode", v, "end") - t0)
                del frames, results
                count["videos"] += 1
                count["frames"] += int(host.shape[0])
                count["pairs"] += len(job.expressions)
                count["files"] += len(paths)
                wr.put(v, paths, blobs)  # waits while 2 * writers videos are queued
                if nxt is None and v + 1 < len(jobs):
                    nxt = take(v + 1, cur)
            if nxt is not None and nxt[3] is not None:
                nxt[3].synchronize()  # invariant 2 for a copy issued and never consumed (a writer failed)
    finally:
        wr.close()  # the prefetcher's threads are joined by now (its `with`), the writers' here
        if up is not None:
            torch.cuda.current_stream(up.device).wait_stream(up.side)
    if wr.error is not None:
        raise wr.error
    return {**count, "seconds": time.perf_counter() - t_start, "busy": dict(tl.busy), "timeline": list(tl.events)}
