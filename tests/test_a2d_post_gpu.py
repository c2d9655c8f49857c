"""The A2D-Sentences / JHMDB-Sentences post-processor on the GPU: tce_a2d_masks_u8 and tce_rle_counts_u32 against the reference
class's fixture (tests/golden/a2d_post_cases.npz) and the restatement (tests/_a2d.py), their access models against the bytes the
launches touch (tests/_footprint.py), and postprocess.A2DSentencesPostProcess on fixture outputs and on the model's own."""
import argparse
import os

import numpy as np
import pytest
import torch

import _a2d
import _footprint as fp
from _util import synth_frames
from tce_rvos_amd import _lib, hazard

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "a2d_post_cases.npz")
SEG = 1024  # TCE_RLE_SEGMENT (include/tce_rvos_eval.h): positions per workgroup of the run-length launches
NAMES = [c[0] for c in _a2d.CASES]


@pytest.fixture(scope="module")
def cases():
    """The fixture, and per case the GPU's own masks (computed once, never modified)."""
    from tce_rvos_amd import ops
    cs = {c["name"]: c for c in _a2d.load_cases(FIXTURE)}
    for c in cs.values():
        c["gpu"] = ops.a2d_masks(c["masks"].cuda(), c["size"], c["orig"])
    torch.cuda.synchronize()
    return cs


def _counts_of(counts, nruns):
    counts, nruns = counts.cpu().numpy(), nruns.cpu().tolist()
    return [counts[p, :nruns[p]].tolist() for p in range(len(nruns))], counts, nruns


# ------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("name", NAMES)
def test_a2d_masks_match_the_reference_class_on_the_fixture(cases, name):
    """Masks equal the reference class's on every non-contested pixel; a second call into a slice on an address = 3 mod 4 gives the
    same bytes and leaves the sentinels around it alone."""
    from tce_rvos_amd import ops
    c = cases[name]
    got = c["gpu"]
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == tuple(c["ref"].shape)
    _a2d.check_masks(got, c["ref"], c["contested"], f"case {name}")
    n = got.numel()
    flat = torch.full((3 + n + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    out = flat[3:3 + n].view(*got.shape)
    assert out.data_ptr() % 4 == 3
    got2 = ops.a2d_masks(c["masks"].cuda(), c["size"], c["orig"], out=out)
    torch.cuda.synchronize()
    assert got2.data_ptr() == out.data_ptr() and torch.equal(out, got)
    assert bool((flat[:3] == 0xEE).all()) and bool((flat[-5:] == 0xEE).all())


@pytest.mark.parametrize("name", NAMES)
def test_rle_counts_of_the_gpu_masks_equal_the_loop(cases, name):
    from tce_rvos_amd import ops
    m = cases[name]["gpu"]
    counts, nruns = ops.rle_counts(m)
    torch.cuda.synchronize()
    assert counts.dtype == torch.int32 and nruns.dtype == torch.int32 and tuple(counts.shape) == (m.shape[0], m.shape[1] * m.shape[2] + 1)
    got, full, nr = _counts_of(counts, nruns)
    host = m.cpu().numpy()
    for p in range(m.shape[0]):
        want = _a2d.rle_counts(host[p])
        print(f"case {name} mask {p}: {nr[p]} runs (loop: {len(want)})")
        assert got[p] == want, (name, p)
        assert not full[p, nr[p]:].any(), "the words behind the counts are zeros"


def _special_masks(H, W):
    """[P,H,W] uint8 built from their column-major bit strings, and the names of the P masks."""
    HW = H * W
    bits = {"all zeros": np.zeros(HW, np.uint8), "all ones": np.ones(HW, np.uint8)}
    b = np.zeros(HW, np.uint8); b[0] = 1; bits["a single 1 at the first position"] = b
    b = np.zeros(HW, np.uint8); b[-1] = 1; bits["a single 1 at the last position"] = b
    bits["checkerboard from 0"] = (np.arange(HW) & 1).astype(np.uint8)
    bits["checkerboard from 1"] = ((np.arange(HW) + 1) & 1).astype(np.uint8)
    if HW > 2 * SEG:
        # boundaries exactly on segment edges (positions SEG and 2*SEG are the first of their segments), segments 0 and 3 without any
        b = np.zeros(HW, np.uint8); b[SEG:2 * SEG] = 1; bits["one run filling segment 1"] = b
        # the last position of segment 0 and the first of segment 1 are both boundaries; a 255 byte counts as a 1
        b = np.zeros(HW, np.uint8); b[SEG - 1] = 255; bits["a single 1 at the last position of segment 0"] = b
        b = np.ones(HW, np.uint8); b[2 * SEG:] = 0; bits["ones up to the edge of segment 2"] = b
        bits["noise"] = (np.random.default_rng(5).random(HW) < 0.3).astype(np.uint8)
    names = list(bits)
    return torch.from_numpy(np.stack([np.ascontiguousarray(bits[k].reshape(W, H).T) for k in names])), names


@pytest.mark.parametrize("H,W", [(5, 7), (37, 91), (1, 1), (1, 2051), (2049, 1)])
def test_rle_counts_special_masks(H, W):
    """37 x 91 = 3367 positions are four segments of 1024 (the last one partial): boundaries at positions 1023, 1024 and 2048 sit
    on both sides of segment edges, and whole segments have none.  5 x 7 is a single partial segment; H is odd in both, so the
    checkerboards alternate at every position: H*W and H*W + 1 runs, the maximum.  1 x 1 is the smallest mask; a single row of 2051
    and a single column of 2049 positions put one position into a third segment."""
    from tce_rvos_amd import ops
    masks, names = _special_masks(H, W)
    counts, nruns = ops.rle_counts(masks.cuda())
    torch.cuda.synchronize()
    got, full, nr = _counts_of(counts, nruns)
    HW = H * W
    for p, k in enumerate(names):
        want = _a2d.rle_counts((masks[p].numpy() != 0).astype(np.uint8))
        print(f"{H}x{W} {k}: {nr[p]} runs")
        assert got[p] == want, (k, got[p][:8], want[:8])
        assert sum(got[p]) == HW and not full[p, nr[p]:].any()
    assert got[0] == [HW] and got[1] == [0, HW]
    assert got[2] == ([0, 1, HW - 1] if HW > 1 else [0, 1]) and got[3] == ([HW - 1, 1] if HW > 1 else [0, 1])
    if H % 2 == 1 or W == 1:
        assert nr[4] == HW and nr[5] == HW + 1
    if HW > 2 * SEG:
        assert got[names.index("one run filling segment 1")] == [SEG, SEG, HW - 2 * SEG]
        assert got[names.index("a single 1 at the last position of segment 0")] == [SEG - 1, 1, HW - SEG]
        assert got[names.index("ones up to the edge of segment 2")] == [0, 2 * SEG, HW - 2 * SEG]


def test_a2d_shape_against_the_restatement_on_the_cpu():
    """N = 5, 80x120 planes, size (320, 475), orig (240, 320): an A2D frame at the reference's 320-pixel evaluation size."""
    from tce_rvos_amd import ops
    _, masks = _a2d.make_inputs(51, 5, (80, 120), "smooth", 8.0)
    size, orig = (320, 475), (240, 320)
    want, v = _a2d.reference_post(masks, size, orig)
    got = ops.a2d_masks(masks.cuda(), size, orig)
    counts, nruns = ops.rle_counts(got)
    torch.cuda.synchronize()
    _a2d.check_masks(got, want, _a2d.contested(v), "A2D shape")
    rl, _, _ = _counts_of(counts, nruns)
    host = got.cpu().numpy()
    for p in range(5):
        assert np.array_equal(_a2d.rle_decode(rl[p], *orig), host[p]), p
    assert rl[0] == _a2d.rle_counts(host[0])


def test_threshold_other_than_one_half(cases):
    from tce_rvos_amd import ops
    c = cases["A"]
    want, v = _a2d.reference_post(c["masks"], c["size"], c["orig"], threshold=0.3)
    got = ops.a2d_masks(c["masks"].cuda(), c["size"], c["orig"], threshold=0.3)
    torch.cuda.synchronize()
    _a2d.check_masks(got, want, _a2d.contested(v, 0.3), "case A at threshold 0.3")
    assert int((got != c["gpu"]).sum()) > 0 and bool((got >= c["gpu"]).all()), "a lower threshold only adds pixels"


def test_rejections():
    from tce_rvos_amd import ops
    pm = torch.zeros(2, 4, 6, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        ops.a2d_masks(pm[..., ::2], (16, 12), (8, 10))
    with pytest.raises(ValueError, match="on the GPU"):
        ops.a2d_masks(pm.cpu(), (16, 24), (8, 10))
    with pytest.raises(ValueError, match="4x"):
        ops.a2d_masks(pm, (17, 24), (8, 10))
    with pytest.raises(ValueError, match="4x"):
        ops.a2d_masks(pm, (16, 25), (8, 10))
    with pytest.raises(ValueError):
        ops.a2d_masks(pm, (16, 24), (8, 10), out=torch.empty(2, 8, 11, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        ops.rle_counts(torch.zeros(2, 4, 6, dtype=torch.uint8, device="cuda")[..., ::2])
    with pytest.raises(ValueError):
        ops.rle_counts(torch.zeros(2, 4, 6, device="cuda"))
    out = ops.a2d_masks(pm, (16, 24), (8, 10))  # all-zero logits: sigmoid 0.5 is not above 0.5
    torch.cuda.synchronize()
    assert not bool(out.any())
    # the C entries themselves, on real buffers
    l = _lib.lib()
    u8 = torch.zeros(2, 8, 10, dtype=torch.uint8, device="cuda")
    cnt, nr, ws = (torch.zeros(2 * 81, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                   torch.zeros(2, dtype=torch.int64, device="cuda"))
    assert l.tce_a2d_masks_u8(None, u8.data_ptr(), 2, 4, 6, 16, 24, 8, 10, 0.5, None) != 0 and b"tce_a2d_masks_u8" in l.tce_last_error()
    assert l.tce_a2d_masks_u8(pm.data_ptr(), None, 2, 4, 6, 16, 24, 8, 10, 0.5, None) != 0
    assert l.tce_a2d_masks_u8(pm.data_ptr(), u8.data_ptr(), 2, 4, 6, 17, 24, 8, 10, 0.5, None) != 0 and b"4x" in l.tce_last_error()
    assert l.tce_a2d_masks_u8(pm.data_ptr(), u8.data_ptr(), 2, 4, 6, 16, 24, 0, 10, 0.5, None) != 0
    assert l.tce_rle_counts_u32(u8.data_ptr(), cnt.data_ptr(), None, ws.data_ptr(), 2, 8, 10, None) != 0 and b"tce_rle_counts_u32" in l.tce_last_error()
    assert l.tce_rle_counts_u32(u8.data_ptr(), cnt.data_ptr(), nr.data_ptr(), None, 2, 8, 10, None) != 0
    assert l.tce_rle_counts_u32(u8.data_ptr(), cnt.data_ptr(), nr.data_ptr(), ws.data_ptr(), 2, 0, 10, None) != 0
    torch.cuda.synchronize()
    assert not bool(u8.any()) and not bool(cnt.any()) and not bool(nr.any())  # a rejected call launches nothing


# ---------------------------------------------------------------------------------------------------------- the footprint
@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(64 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


def _masks_case(S, N, h, w, fh, fw, H0, W0, shift):
    pm = S.randn("masks", (N, h * w), scale=3.0)
    total = N * H0 * W0
    raw = S.alloc("out", (shift + total + 3,), dtype=torch.uint8)
    out = raw.data_ptr() + shift

    def fn():
        _lib.check(_lib.lib().tce_a2d_masks_u8(pm.data_ptr(), out, N, h, w, fh, fw, H0, W0, 0.5, torch.cuda.current_stream().cuda_stream),
                   "tce_a2d_masks_u8")
    fn.check = lambda: (raw, pm)
    return fn


MASKS_FOOTPRINT = [
    ("up_5x18x25_72x100_to_111x150", dict(N=5, h=18, w=25, fh=72, fw=100, H0=111, W0=150, shift=0)),
    ("down_cropped_odd_address_odd_w0_3x23x40_90x157_to_87x145", dict(N=3, h=23, w=40, fh=90, fw=157, H0=87, W0=145, shift=3)),
    ("tiny_2x3x4_9x13_to_5x7_address_1", dict(N=2, h=3, w=4, fh=9, fw=13, H0=5, W0=7, shift=1)),
]


@pytest.mark.parametrize("tag,kw", MASKS_FOOTPRINT, ids=[c[0] for c in MASKS_FOOTPRINT])
def test_a2d_masks_footprint(slab, tag, kw):
    """W, O and R of tests/_footprint.py, no exemptions: nothing outside `out` is written (the bytes around an oddly placed plane
    included), every output byte is written, and the result depends on no byte outside the N mask planes."""
    from tce_rvos_amd import ops
    info = fp.check_case(slab, lambda S: _masks_case(S, **kw), fp.recorder("tce_a2d_masks_u8"), props="WOR", sync=torch.cuda.synchronize, label=tag)
    print(f"{tag}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']} untouched-in-buffers {info['pad_bytes']}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == []
    assert info["read_bytes"] == kw["N"] * kw["h"] * kw["w"] * 4
    assert info["written_bytes"] == kw["N"] * kw["H0"] * kw["W0"]
    slab.begin(0)
    fn = _masks_case(slab, **kw)
    fn()
    raw, pm = fn.check()
    sh, total = kw["shift"], kw["N"] * kw["H0"] * kw["W0"]
    want = ops.a2d_masks(pm.reshape(kw["N"], kw["h"], kw["w"]).clone(), (kw["fh"], kw["fw"]), (kw["H0"], kw["W0"]))
    torch.cuda.synchronize()
    assert torch.equal(raw[sh:sh + total], want.reshape(-1))


RLE_FOOTPRINT = [
    ("three_masks_87x145_13_segments", dict(P=3, H=87, W=145)),
    ("two_masks_5x7_one_segment", dict(P=2, H=5, W=7)),
]


def _rle_case(S, P, H, W):
    m = S.randint("masks", (P, H * W), 0, 2, dtype=torch.uint8)
    counts = S.alloc("counts", (P, H * W + 1), dtype=torch.int32)
    nruns = S.alloc("nruns", (P,), dtype=torch.int32)
    ws = S.alloc("ws", (_lib.lib_raw().tce_rle_ws_bytes(P, H, W) // 8,), dtype=torch.int64)

    def fn():
        _lib.check(_lib.lib().tce_rle_counts_u32(m.data_ptr(), counts.data_ptr(), nruns.data_ptr(), ws.data_ptr(), P, H, W,
                                                 torch.cuda.current_stream().cuda_stream), "tce_rle_counts_u32")
    fn.check = lambda: (m, counts, nruns)
    return fn


@pytest.mark.parametrize("tag,kw", RLE_FOOTPRINT, ids=[c[0] for c in RLE_FOOTPRINT])
def test_rle_counts_footprint(slab, tag, kw):
    """W, O and R with no exemption: every word of counts is written (the counts, then zeros), so the whole of counts and nruns is
    held to O and compared under R; ws is scratch (R fills it before the run: the second launch must not consume a record the
    first did not write)."""
    info = fp.check_case(slab, lambda S: _rle_case(S, **kw), fp.recorder("tce_rle_counts_u32"), scratch=("ws",), props="WOR",
                         sync=torch.cuda.synchronize, label=tag)
    print(f"{tag}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == []
    P, HW = kw["P"], kw["H"] * kw["W"]
    wsb = P * -(-HW // SEG) * 8
    assert info["read_bytes"] == P * HW + wsb and info["written_bytes"] == P * (HW + 1) * 4 + 4 * P + wsb
    slab.begin(0)
    fn = _rle_case(slab, **kw)
    fn()
    m, counts, nruns = fn.check()
    torch.cuda.synchronize()
    got, _, _ = _counts_of(counts, nruns)
    host = m.cpu().numpy().reshape(P, kw["H"], kw["W"])
    for p in range(P):
        assert got[p] == _a2d.rle_counts(host[p]), p


# ------------------------------------------------------------------------------------------------------- the post-processor
def _outputs(cs):
    """Fixture cases (same N, same plane) as one batch: pred_logits [B,1,N,1], pred_masks [B,1,N,h,w]."""
    lg = torch.stack([c["logits"] for c in cs]).view(len(cs), 1, -1, 1).cuda()
    pm = torch.stack([c["masks"] for c in cs]).unsqueeze(1).cuda()
    return {"pred_logits": lg, "pred_masks": pm}


def _check_result(r, c, exact):
    N, (H0, W0) = c["masks"].shape[0], c["orig"]
    assert set(r) == {"scores", "masks", "rle_masks"}
    assert r["scores"].dtype == torch.float32 and r["scores"].is_cuda and tuple(r["scores"].shape) == (N,)
    assert r["masks"].dtype == torch.uint8 and r["masks"].is_cuda and tuple(r["masks"].shape) == (N, 1, H0, W0)
    assert float((r["scores"].cpu() - c["scores"]).abs().max()) <= 1e-6
    _a2d.check_masks(r["masks"][:, 0], c["ref"], c["contested"], f"case {c['name']} through the class")
    assert torch.equal(r["masks"][:, 0], c["gpu"])
    assert isinstance(r["rle_masks"], list) and len(r["rle_masks"]) == N
    own = r["masks"][:, 0].cpu().numpy()
    for n, e in enumerate(r["rle_masks"]):
        assert set(e) == {"size", "counts"} and e["size"] == [H0, W0] and isinstance(e["counts"], bytes)
        assert e["counts"] == _a2d.rle_string(_a2d.rle_counts(own[n])), (c["name"], n)
        if exact:
            assert e["counts"] == c["rle"][n], (c["name"], n)


@pytest.mark.parametrize("name", NAMES)
def test_postprocess_class_on_fixture_outputs(cases, name):
    """Key set, dtypes, shapes, scores within 1e-6; the strings of C and D (no contested pixel) equal the fixture's byte for byte,
    those of A and B are the loop's strings of the class's own masks."""
    from tce_rvos_amd.postprocess import A2DSentencesPostProcess
    c = cases[name]
    post = A2DSentencesPostProcess(threshold=0.9)  # binarises at 0.5 all the same, as the reference class
    res = post(_outputs([c]), torch.tensor([c["orig"]]), torch.tensor([c["size"]]))
    assert len(res) == 1 and post.threshold == 0.9
    _check_result(res[0], c, exact=name in ("C", "D"))


def test_postprocess_class_two_samples_and_list_form(cases):
    """B = 2 with different size / orig in one call (case C and the first 3 of case A's 5 queries: one batch needs one N); sizes on
    the GPU, as engine.py stacks them; and the list-of-dicts form of forward_group."""
    from tce_rvos_amd.postprocess import A2DSentencesPostProcess
    a = dict(cases["A"])
    for k in ("logits", "masks", "scores", "ref", "contested", "gpu"):
        a[k] = a[k][:3]
    a["rle"] = a["rle"][:3]
    c = cases["C"]
    post = A2DSentencesPostProcess()
    orig, size = torch.tensor([a["orig"], c["orig"]]).cuda(), torch.tensor([a["size"], c["size"]]).cuda()
    res = post(_outputs([a, c]), orig, size)
    assert len(res) == 2
    _check_result(res[0], a, exact=False)
    _check_result(res[1], c, exact=True)
    res2 = post([_outputs([a]), _outputs([c])], [a["orig"], c["orig"]], [torch.tensor(a["size"]), torch.tensor(c["size"])])
    assert len(res2) == 2
    for r, r2 in zip(res, res2):
        assert torch.equal(r["masks"], r2["masks"]) and torch.equal(r["scores"], r2["scores"]) and r["rle_masks"] == r2["rle_masks"]


# ------------------------------------------------------------------------------------------------------------- end to end
def _args(backbone, **kw):
    return argparse.Namespace(backbone=backbone, with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1, **kw)


def test_end_to_end_build_model_third_value_post_processes_the_models_output():
    """Small Swin-T, T = 3 frames of 72x100, valid_indices = 1, dataset_file = 'a2d': what engine.evaluate_a2d does up to its
    predictions.append."""
    from tce_rvos_amd import build_model, load_synth_weights, ops
    from tce_rvos_amd.postprocess import A2DSentencesPostProcess
    model, _, post = build_model(_args("swin_t_p4w7", dataset_file="a2d", threshold=0.5))
    assert isinstance(post, A2DSentencesPostProcess)
    model = model.cuda().eval()
    load_synth_weights(model, 31)
    model.repack()
    H, W, orig = 72, 100, (111, 150)
    frames = synth_frames(3, H, W, 92).cuda()
    targets = [{"size": torch.tensor([H, W]), "orig_size": torch.tensor(orig), "valid_indices": torch.tensor(1)}]
    outputs = model([frames], ["the left zebra"], targets)
    N = outputs["pred_masks"].shape[2]
    assert tuple(outputs["pred_masks"].shape) == (1, 1, N, 18, 25)
    orig_target_sizes = torch.stack([t["orig_size"] for t in targets], dim=0)   # engine.py:310-311
    target_sizes = torch.stack([t["size"] for t in targets], dim=0)
    processed = post(outputs, orig_target_sizes, target_sizes)
    assert len(processed) == 1
    p = processed[0]
    pm = outputs["pred_masks"][0, 0].cpu()
    want, v = _a2d.reference_post(pm, (H, W), orig)
    _a2d.check_masks(p["masks"][:, 0], want, _a2d.contested(v), "end to end")
    assert float((p["scores"].cpu() - outputs["pred_logits"][0, 0, :, 0].cpu().sigmoid()).abs().max()) <= 1e-6
    own = p["masks"][:, 0].cpu().numpy()
    for s, rle_mask in zip(p["scores"].cpu().tolist(), p["rle_masks"]):   # engine.py:314-319 reads exactly these
        assert isinstance(s, float) and rle_mask["size"] == list(orig)
    for n in range(N):
        assert np.array_equal(_a2d.rle_decode(_a2d.rle_from_string(p["rle_masks"][n]["counts"]), *orig), own[n]), n
    # the same stage recorded as a launch program: its entries, in order, with no conflicting pair
    with hazard.recording() as rec:
        again = post(outputs, orig_target_sizes, target_sizes)
    assert [x.name for x in rec.launches] == ["tce_sigmoid_f32", "tce_a2d_masks_u8", "tce_rle_counts_u32"]
    assert rec.analyse().clean
    assert torch.equal(again[0]["masks"], p["masks"]) and again[0]["rle_masks"] == p["rle_masks"]
    # ... and captured: the two entries allocate nothing and never synchronise, so they replay from a graph on new logits
    src = outputs["pred_masks"][0, 0].clone()
    out = torch.zeros(N, *orig, dtype=torch.uint8, device="cuda")
    counts, nruns = ops.rle_counts(ops.a2d_masks(src, (H, W), orig, out=out))
    ws = torch.zeros(_lib.lib().tce_rle_ws_bytes(N, *orig) // 8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.a2d_masks(src, (H, W), orig, out=out)
        ops.rle_counts(out, counts=counts, nruns=nruns, ws=ws)
    src.copy_(-src)
    g.replay()
    torch.cuda.synchronize()
    want2, v2 = _a2d.reference_post(-pm, (H, W), orig)
    _a2d.check_masks(out, want2, _a2d.contested(v2), "end to end, replayed on the negated logits")
    got, _, _ = _counts_of(counts, nruns)
    host = out.cpu().numpy()
    for n in range(N):
        assert got[n] == _a2d.rle_counts(host[n]), n
