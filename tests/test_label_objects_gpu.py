"""Ref-DAVIS label maps on the GPU: tce_label_objects_u8 against the reference caller's restatement (tests/_davis.py) on the
committed fixture and on one full-size chunk, its access model against the bytes the two launches touch (tests/_footprint.py), and
video.run_video_objects against the restatement applied to its own forwards and against run_video_expressions."""
import argparse
import os

import numpy as np
import pytest
import torch

import _davis
import _footprint as fp
from _util import synth_frames
from tce_rvos_amd import _lib

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "davis_label_cases.npz")


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", [c[0] for c in _davis.CASES])
def test_label_objects_matches_the_reference_caller_on_the_fixture(name):
    """Labels equal the fixture on every non-contested pixel and are <= n everywhere; best queries equal; contested share <= 1 %."""
    from tce_rvos_amd import ops
    c = next(c for c in _davis.load_cases(FIXTURE) if c["name"] == name)
    lg, pm = c["logits"].cuda(), c["masks"].cuda()
    labels, best = ops.label_objects(list(lg), list(pm), c["size"])     # a list of views: the pointers go into the table
    labels2, best2 = ops.label_objects(lg, pm, c["size"])               # stacked
    torch.cuda.synchronize()
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == tuple(c["labels"].shape) and best.dtype == torch.int32
    assert torch.equal(best.cpu(), c["best"]), (best.cpu().tolist(), c["best"].tolist())
    _davis.check_labels(labels, c["labels"], c["contested"], c["n"], f"case {name}")
    assert torch.equal(labels, labels2) and torch.equal(best, best2)
    # every object's query is the one tce_select_masks_u8 picks, and a one-object map is that entry's mask (the same operations)
    for k in range(c["n"]):
        m, b = ops.select_masks(lg[k], pm[k], c["size"])
        one, b1 = ops.label_objects([lg[k]], [pm[k]], c["size"])
        assert int(b) == int(best[k]) == int(b1)
        ref1, _, cont1 = _davis.reference_labels([c["logits"][k]], [c["masks"][k]], c["size"])
        assert not bool(((one.cpu() != m.cpu()) & ~cont1).any())
        _davis.check_labels(one, ref1, cont1, 1, f"case {name} object {k} alone")


def test_label_objects_full_size_chunk():
    """n = 5, T = 32, 120x214 -> 480x854 (a 32-frame DAVIS chunk), against the restatement run with torch on the CPU; written into a
    slice of a longer label map that starts on an odd address."""
    from tce_rvos_amd import ops
    n, T, Q, h, w, H0, W0 = 5, 32, 5, 120, 214, 480, 854
    g = torch.Generator().manual_seed(36)
    logits = torch.randn(n, T, Q, 1, generator=g)
    masks = torch.randn(n, T, Q, h, w, generator=g) * 3
    want, best_ref, contested = _davis.reference_labels(list(logits), list(masks), (H0, W0))
    lg, pm = [t.cuda() for t in logits], [t.cuda() for t in masks]   # n separate allocations
    labels, best = ops.label_objects(lg, pm, (H0, W0))
    torch.cuda.synchronize()
    assert torch.equal(best.cpu(), best_ref)
    _davis.check_labels(labels, want, contested, n, "full-size chunk")
    flat = torch.full((3 + T * H0 * W0 + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    out = flat[3:3 + T * H0 * W0].view(T, H0, W0)
    assert out.data_ptr() % 4 == 3
    got, _ = ops.label_objects(lg, pm, (H0, W0), out=out, best_out=torch.empty(n, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, labels)
    assert bool((flat[:3] == 0xEE).all()) and bool((flat[-5:] == 0xEE).all())


def test_label_objects_rejects_what_it_cannot_run():
    from tce_rvos_amd import ops
    lg, pm = torch.zeros(2, 3, 1, device="cuda"), torch.zeros(2, 3, 4, 6, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        ops.label_objects([lg], [pm[..., ::2]], (8, 10))
    with pytest.raises(ValueError, match="on the GPU"):
        ops.label_objects([lg, lg.cpu()], [pm, pm], (8, 10))
    with pytest.raises(ValueError, match="1..16 objects"):
        ops.label_objects([lg] * 17, [pm] * 17, (8, 10))
    labels, best = ops.label_objects([lg] * 16, [pm] * 16, (8, 10))  # 16 is the limit; all-zero logits: score 0.5 beats 0.1, object 0
    torch.cuda.synchronize()
    assert bool((labels == 1).all()) and best.cpu().tolist() == [0] * 16
    # the C entry itself: n out of range, a missing best_query
    t = (_lib.LabelObj * 17)()
    for o in t:
        o.logits, o.masks = lg.data_ptr(), pm.data_ptr()
    l = _lib.lib()
    assert l.tce_label_objects_u8(t, 17, labels.data_ptr(), best.data_ptr(), 2, 3, 1, 4, 6, 8, 10, 0.5, 0.1, None) != 0
    assert b"tce_label_objects_u8" in l.tce_last_error()
    assert l.tce_label_objects_u8(t, 0, labels.data_ptr(), best.data_ptr(), 2, 3, 1, 4, 6, 8, 10, 0.5, 0.1, None) != 0
    assert l.tce_label_objects_u8(t, 2, labels.data_ptr(), None, 2, 3, 1, 4, 6, 8, 10, 0.5, 0.1, None) != 0


# ---------------------------------------------------------------------------------------------------------- the footprint
@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(64 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


def _label_case(S, n, T, Q, K, h, w, H0, W0, order, shift):
    """Every device buffer of the call in the slab, objects allocated in index order and listed in `order`; labels start `shift`
    bytes into their buffer.  The table is a host array, read by the entry point at launch time: it stays outside the slab."""
    bufs = [(S.randn(f"logits{k}", (T * Q, K)), S.randn(f"masks{k}", (T * Q, h * w), scale=3.0)) for k in range(n)]
    total = T * H0 * W0
    raw = S.alloc("labels", (shift + total + 3,), dtype=torch.uint8)
    bq = S.alloc("best_query", (n,), dtype=torch.int32)
    table = (_lib.LabelObj * n)()
    for o, k in zip(table, order):
        o.logits, o.masks = bufs[k][0].data_ptr(), bufs[k][1].data_ptr()
    labels = raw.data_ptr() + shift

    def fn():
        _lib.check(_lib.lib().tce_label_objects_u8(table, n, labels, bq.data_ptr(), T, Q, K, h, w, H0, W0, 0.5, 0.1,
                                                   torch.cuda.current_stream().cuda_stream), "tce_label_objects_u8")
    fn.check = lambda: (raw, bq, bufs)
    return fn


FOOTPRINT_CASES = [
    ("one_object_3x5x1_18x25_to_72x100", dict(n=1, T=3, Q=5, K=1, h=18, w=25, H0=72, W0=100, order=(0,), shift=0)),
    ("three_objects_mixed_order_odd_w0_2x3x2_9x13_to_37x51", dict(n=3, T=2, Q=3, K=2, h=9, w=13, H0=37, W0=51, order=(2, 0, 1), shift=0)),
    ("four_objects_odd_address_2x70x1_23x40_to_97x151", dict(n=4, T=2, Q=70, K=1, h=23, w=40, H0=97, W0=151, order=(1, 3, 0, 2), shift=1)),
]


@pytest.mark.parametrize("tag,kw", FOOTPRINT_CASES, ids=[c[0] for c in FOOTPRINT_CASES])
def test_label_objects_footprint(slab, tag, kw):
    """W, O and R of tests/_footprint.py, no exemptions: nothing outside labels / best_query is written (the pad bytes around an
    oddly placed label map included), every label byte and every best_query word is written, and the result depends on no byte
    outside the n logits and n masks blocks."""
    from tce_rvos_amd import ops
    info = fp.check_case(slab, lambda S: _label_case(S, **kw), fp.recorder("tce_label_objects_u8"), props="WOR", sync=torch.cuda.synchronize, label=tag)
    print(f"{tag}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']} untouched-in-buffers {info['pad_bytes']}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == []
    n, T = kw["n"], kw["T"]
    assert info["written_bytes"] == T * kw["H0"] * kw["W0"] + 4 * n
    assert info["read_bytes"] == n * T * kw["Q"] * (kw["K"] + kw["h"] * kw["w"]) * 4
    # the launch under the slab's last state computes what the op computes on the same values
    slab.begin(0)
    fn = _label_case(slab, **kw)
    fn()
    raw, bq, bufs = fn.check()
    sh, total = kw["shift"], T * kw["H0"] * kw["W0"]
    lg = [bufs[k][0].reshape(T, kw["Q"], kw["K"]).clone() for k in kw["order"]]
    pm = [bufs[k][1].reshape(T, kw["Q"], kw["h"], kw["w"]).clone() for k in kw["order"]]
    want, best = ops.label_objects(lg, pm, (kw["H0"], kw["W0"]))
    torch.cuda.synchronize()
    assert torch.equal(raw[sh:sh + total], want.reshape(-1)) and torch.equal(bq, best)
    ref, best_ref, contested = _davis.reference_labels([t.cpu() for t in lg], [t.cpu() for t in pm], (kw["H0"], kw["W0"]))
    assert torch.equal(best.cpu(), best_ref)
    _davis.check_labels(want, ref, contested, n, tag)


# ------------------------------------------------------------------------------------------------------------- the driver
def _args(backbone):
    return argparse.Namespace(backbone=backbone, with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)


@pytest.fixture(scope="module")
def model():
    from tce_rvos_amd import build_model, load_synth_weights
    m, _, _ = build_model(_args("swin_t_p4w7"))
    m = m.cuda().eval()
    load_synth_weights(m, 31)
    m.repack()
    return m


@pytest.mark.parametrize("mixed", [False, True])
def test_run_video_objects(model, mixed):
    """Small Swin-T, 7 frames in chunks of 4 (a shorter last one), 4 captions of two token lengths, three overlapping sets."""
    from tce_rvos_amd.video import run_video_expressions, run_video_objects
    H, W, H0, W0 = 96, 128, 181, 239
    N, step = 7, 4
    frames = synth_frames(N, H, W, 90).cuda()
    caps = ["the left zebra", "a person walking a dog", "the right zebra", "a dog chasing the ball"]
    lens = [int(model._tokenise([c], frames.device)[0].shape[1]) for c in caps]
    assert lens[0] == lens[2] != lens[1] == lens[3], lens
    sets = [[0, 1, 2, 3], [2, 0], [1]]
    seen = []  # (first frame of the clip, token rows, outputs) of every forward_group call
    orig = model.forward_group

    def recording(clips, tok, *a, **k):
        outs = orig(clips, tok, *a, **k)
        assert all(c is clips[0] for c in clips) and k.get("ragged", False) == mixed
        seen.append((int(clips[0].shape[0]), tok.cpu(), [{kk: o[kk][0].cpu() for kk in ("pred_logits", "pred_masks", "pred_boxes")} for o in outs]))
        return outs
    model.forward_group = recording
    try:
        res = run_video_objects(model, frames, caps, (H0, W0), clip_size=step, object_sets=sets, max_group=4, mixed_lengths=mixed)
    finally:
        del model.forward_group
    torch.cuda.synchronize()
    # every caption once per chunk: 2 chunks x (2 length buckets | 1 mixed group), 4 caption rows per chunk in all
    per_chunk = 1 if mixed else 2
    assert len(seen) == 2 * per_chunk
    assert [s[0] for s in seen] == [4] * per_chunk + [3] * per_chunk, "the chunk loop is the outer loop"
    assert [sum(s[1].shape[0] for s in seen[c * per_chunk:(c + 1) * per_chunk]) for c in range(2)] == [4, 4]
    from tce_rvos_amd.video import plan_object_forwards
    _, plan = plan_object_forwards(lens, N, step, sets, 4, mixed)
    assert len(plan) == len(seen)
    held = {}  # (chunk start, caption) -> that forward's outputs
    for (lo, hi, grp), (T, tok, outs) in zip(plan, seen):
        assert T == hi - lo and tok.shape[0] == len(grp) == len(outs)
        for i, o in zip(grp, outs):
            assert (lo, i) not in held
            held[(lo, i)] = o
    assert len(held) == 2 * len(caps)

    ref = run_video_expressions(model, frames, caps, (H0, W0), clip_size=step, max_group=4, mixed_lengths=mixed)
    assert len(res) == len(sets)
    for s, r in zip(sets, res):
        n = len(s)
        assert r["labels"].dtype == torch.uint8 and tuple(r["labels"].shape) == (N, H0, W0)
        assert tuple(r["best_query"].shape) == (n, 2) and r["best_query"].dtype == torch.int32
        assert tuple(r["pred_logits"].shape)[:2] == (n, N) and tuple(r["pred_boxes"].shape) == (n, N, 4)
        # labels = the reference caller's restatement on the outputs of these very forwards, chunk by chunk
        want, cont = [], []
        for c, lo in enumerate((0, 4)):
            lab, best, ct = _davis.reference_labels([held[(lo, i)]["pred_logits"] for i in s], [held[(lo, i)]["pred_masks"] for i in s], (H0, W0))
            assert torch.equal(r["best_query"][:, c].cpu(), best), (s, c)
            want.append(lab)
            cont.append(ct)
        want, cont = torch.cat(want, 0), torch.cat(cont, 0)
        print(f"set {s}: label histogram {np.bincount(r['labels'].cpu().numpy().ravel(), minlength=n + 1).tolist()}")
        _davis.check_labels(r["labels"], want, cont, n, f"mixed={mixed} set {s}")
        # per object what run_video_expressions returns for its caption, exactly
        for k, i in enumerate(s):
            assert torch.equal(r["best_query"][k], ref[i]["best_query"]), (s, k)
            assert torch.equal(r["pred_logits"][k], ref[i]["pred_logits"]), (s, k)
            assert torch.equal(r["pred_boxes"][k], ref[i]["pred_boxes"]), (s, k)
        any_obj = torch.stack([ref[i]["masks"] for i in s], 0).amax(0)
        bg_differs = ((r["labels"] == 0) != (any_obj == 0)).cpu() & ~cont
        assert not bool(bg_differs.any()), (s, int(bg_differs.sum()))
        if n == 1:
            assert not bool(((r["labels"] != ref[s[0]]["masks"]).cpu() & ~cont).any())
    # the sets share forwards: object 0 of set 1 is object 2 of set 0
    assert torch.equal(res[1]["best_query"][0], res[0]["best_query"][2]) and torch.equal(res[1]["pred_boxes"][1], res[0]["pred_boxes"][0])
    assert torch.equal(res[2]["pred_logits"][0], res[0]["pred_logits"][1])


def test_run_video_objects_default_set_and_annotator_sets(model):
    """The default is one map of all captions in order; the four DAVIS annotator sets of 8 expressions give four two-object maps."""
    from tce_rvos_amd.video import davis_annotator_sets, run_video_objects
    H, W, H0, W0 = 96, 128, 120, 160
    frames = synth_frames(3, H, W, 91).cuda()
    caps = ["the left zebra", "the right zebra", "the small dog", "a dog running", "the big zebra", "the far zebra", "the near dog", "a zebra eating"]
    one = run_video_objects(model, frames, caps[:3], (H0, W0), clip_size=None)
    assert len(one) == 1 and tuple(one[0]["labels"].shape) == (3, H0, W0) and tuple(one[0]["best_query"].shape) == (3, 1)
    assert int(one[0]["labels"].max()) <= 3
    four = run_video_objects(model, frames, caps, (H0, W0), clip_size=None, object_sets=davis_annotator_sets(len(caps)), max_group=8)
    assert len(four) == 4
    for anno, r in enumerate(four):
        assert tuple(r["labels"].shape) == (3, H0, W0) and int(r["labels"].max()) <= 2 and tuple(r["best_query"].shape) == (2, 1)
    with pytest.raises(ValueError):
        run_video_objects(model, frames, caps, (H0, W0), object_sets=[[0, 9]])
