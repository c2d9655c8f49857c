"""Ref-DAVIS J&F scoring on the GPU: tce_jf_counts_i32 against the NumPy restatement of the reference's davis2017/metrics.py
(tests/_jf.py; its results for cases A-G are committed as tests/golden/jf_cases.npz), score.score_video on top of it, the access
model against the bytes the launches touch (tests/_footprint.py).  Every comparison is integer or bit equality."""
import os

import numpy as np
import pytest
import torch

import _footprint as fp
import _jf
from tce_rvos_amd import _lib, hazard, score  # noqa: F401  (without the scoring module nothing here can run)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jf_cases.npz")
NAMES = [c[0] for c in _jf.CASES]
COLS = ("inters", "union", "n_fg", "n_gt", "fg_match", "gt_match")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def cases():
    """The fixture, the maps on the device, and per case the GPU's own counts (computed once, never modified)."""
    from tce_rvos_amd import ops
    cs = _jf.load_cases(FIXTURE)
    for c in cs.values():
        c["pred_gpu"], c["gt_gpu"] = torch.from_numpy(c["pred"]).cuda(), torch.from_numpy(c["gt"]).cuda()
        c["gpu"] = ops.jf_counts(c["pred_gpu"], c["gt_gpu"], c["n"], c["radius"])
    torch.cuda.synchronize()
    return cs


def _assert_counts(got, want, what):
    got, want = np.asarray(got.cpu() if torch.is_tensor(got) else got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    print(f"{what}: {want.shape[0]} objects x {want.shape[1]} frames, column sums {got.sum(axis=(0, 1)).tolist()} "
          f"(reference {want.sum(axis=(0, 1)).tolist()}), {len(bad)} words differ")
    for k, t, j in bad[:8]:
        print(f"  object {k} frame {t} {COLS[j]}: got {got[k, t, j]}, reference {want[k, t, j]}")
    assert not len(bad), f"{what}: {len(bad)} counts differ from the reference"


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", NAMES)
def test_jf_counts_equal_the_reference_on_the_fixture(cases, name):
    c = cases[name]
    got = c["gpu"]
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == c["counts"].shape
    _assert_counts(got, c["counts"], f"case {name}")


def test_jf_counts_full_size_against_the_restatement_on_the_cpu():
    """T = 2, n = 3, 480 x 854, radius 8: a DAVIS frame at its own boundary radius."""
    from tce_rvos_amd import ops, score
    name, seed, T, n, H, W, radius, kind = _jf.FULL
    assert score.boundary_radius(H, W) == radius
    pred, gt = _jf.make_case(_jf.FULL)
    got = ops.jf_counts(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), n, radius)
    want, J, F = _jf.reference(pred, gt, n, radius)
    torch.cuda.synchronize()
    _assert_counts(got, want, "full size")
    assert int(want[..., 2].min()) > 0 and int(want[..., 4].min()) > 0  # every object has a boundary and matches in every frame
    J2, F2 = score.jf_from_counts(got)
    assert np.array_equal(_bits(J2), _bits(J)) and np.array_equal(_bits(F2), _bits(F))


def test_radius_zero_and_the_large_radii():
    """radius 0 (a pixel matches only itself) and TCE_JF_MAX_RADIUS on case B's maps -- the two ends of the half-width table, the
    second with a halo wider than the plane -- and the 4K radius, 36, on sparse blobs over 100 x 200 (radii above 28 fetch a row
    per wavefront pass instead of two)."""
    from tce_rvos_amd import ops
    case = _jf.CASES[1]
    todo = [(_jf.make_case(case), case[3], 0, "case B"), (_jf.make_case(case), case[3], 40, "case B")]
    wide = ("R36", 79, 1, 2, 100, 200, 36, "sparse")
    todo.append((_jf.make_case(wide), wide[3], wide[6], "sparse blobs 100x200"))
    for (pred, gt), n, radius, what in todo:
        got = ops.jf_counts(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), n, radius)
        want, _, _ = _jf.reference(pred, gt, n, radius)
        torch.cuda.synchronize()
        _assert_counts(got, want, f"{what} at radius {radius}")
        assert int(want[..., 2].sum()) > 0 and int(want[..., 3].sum()) > 0


def test_prefilled_buffers_and_a_second_call_give_the_same_words(cases):
    """counts and ws pre-filled with 0xFF bytes: every word of counts is written and nothing of ws is consumed unwritten; a second
    call into the same buffers gives the same words."""
    from tce_rvos_amd import ops
    for name in ("B", "G"):
        c = cases[name]
        T, H, W = c["pred"].shape
        counts = torch.full((c["n"], T, 6), -1, dtype=torch.int32, device="cuda")
        ws = torch.full((_lib.lib().tce_jf_ws_bytes(T, c["n"], H, W, c["radius"]) // 8,), -1, dtype=torch.int64, device="cuda")
        out = ops.jf_counts(c["pred_gpu"], c["gt_gpu"], c["n"], c["radius"], counts=counts, ws=ws)
        torch.cuda.synchronize()
        assert out.data_ptr() == counts.data_ptr() and torch.equal(counts, c["gpu"]), name
        first = counts.clone()
        ops.jf_counts(c["pred_gpu"], c["gt_gpu"], c["n"], c["radius"], counts=counts, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(counts, first), name
        assert torch.equal(ops.jf_counts(c["pred_gpu"], c["gt_gpu"], c["n"], c["radius"]), first), name


def test_maps_on_odd_addresses(cases):
    """The label planes start 1 and 3 bytes into their allocations (a slice of a larger uint8 buffer): the same counts."""
    from tce_rvos_amd import ops
    c = cases["C"]
    numel = c["pred"].size
    a = torch.zeros(numel + 8, dtype=torch.uint8, device="cuda")
    b = torch.zeros(numel + 8, dtype=torch.uint8, device="cuda")
    p, g = a[1:1 + numel].view(*c["pred"].shape), b[3:3 + numel].view(*c["gt"].shape)
    p.copy_(c["pred_gpu"])
    g.copy_(c["gt_gpu"])
    assert p.data_ptr() % 4 == 1 and g.data_ptr() % 4 == 3
    got = ops.jf_counts(p, g, c["n"], c["radius"])
    torch.cuda.synchronize()
    _assert_counts(got, c["counts"], "case C on odd addresses")


def test_graph_capture_replays_on_new_inputs(cases):
    """One call captured by torch.cuda.graph; the maps are then overwritten in place and the graph replayed: it equals the eager
    call on the new maps (the entry allocates nothing and never synchronises)."""
    from tce_rvos_amd import ops
    c = cases["G"]
    T, H, W = c["pred"].shape
    n, radius = c["n"], c["radius"]
    pred, gt = c["pred_gpu"].clone(), c["gt_gpu"].clone()
    counts = torch.zeros(n, T, 6, dtype=torch.int32, device="cuda")
    ws = torch.zeros(_lib.lib().tce_jf_ws_bytes(T, n, H, W, radius) // 8, dtype=torch.int64, device="cuda")
    ops.jf_counts(pred, gt, n, radius, counts=counts, ws=ws)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.jf_counts(pred, gt, n, radius, counts=counts, ws=ws)
    pred.copy_(c["gt_gpu"].flip(2))   # new maps: the annotation mirrored as the prediction, the old prediction as the annotation
    gt.copy_(c["pred_gpu"])
    counts.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    eager = ops.jf_counts(pred.clone(), gt.clone(), n, radius)
    torch.cuda.synchronize()
    assert torch.equal(counts, eager) and not torch.equal(counts, c["gpu"])
    want, _, _ = _jf.reference(pred.cpu().numpy(), gt.cpu().numpy(), n, radius)
    _assert_counts(counts, want, "case G mirrored, replayed")


def test_hazard_recording_lists_the_one_entry(cases):
    from tce_rvos_amd import ops
    c = cases["B"]
    with hazard.recording() as rec:
        got = ops.jf_counts(c["pred_gpu"], c["gt_gpu"], c["n"], c["radius"])
    torch.cuda.synchronize()
    assert [x.name for x in rec.launches] == ["tce_jf_counts_i32"]
    assert rec.analyse().clean and torch.equal(got, c["gpu"])


# ------------------------------------------------------------------------------------------------------------ score_video
def test_score_video_on_case_g_equals_the_reference_bit_for_bit(cases):
    from tce_rvos_amd import score
    c = cases["G"]
    res = score.score_video(c["pred_gpu"], c["gt_gpu"], drop_first_last=False)  # n=None: read from the first annotation
    assert res["n"] == 3 and res["radius"] == score.boundary_radius(150, 300) == 3
    # the fixture's G is at radius 8 (bound_th >= 1 is taken as the radius itself, metrics.py:77)
    res = score.score_video(c["pred_gpu"], c["gt_gpu"], bound_th=8, drop_first_last=False)
    assert res["n"] == 3 and res["radius"] == 8
    assert np.array_equal(res["counts"], c["counts"])
    assert np.array_equal(_bits(res["J"]), _bits(c["J"])) and np.array_equal(_bits(res["F"]), _bits(c["F"]))
    for k in range(3):
        for key, v in zip(("JM", "JR", "JD"), score.db_statistics(c["J"][k])):
            assert _bits(res[key][k]) == _bits(v), (key, k)
        for key, v in zip(("FM", "FR", "FD"), score.db_statistics(c["F"][k])):
            assert _bits(res[key][k]) == _bits(v), (key, k)
    s = score.summarize([res])
    assert s["J-Mean"] == np.mean(res["JM"]) and s["J&F-Mean"] == (np.mean(res["JM"]) + np.mean(res["FM"])) / 2.


def test_score_video_drops_the_first_and_last_frame_and_ignores_void(cases):
    """Four frames in, frames 1:-1 scored (evaluation.py:85); n comes from the FIRST frame, whose 255 pixels count as 0."""
    from tce_rvos_amd import score
    c = cases["C"]
    pred = torch.cat([c["pred_gpu"], c["pred_gpu"]])  # frames 0 1 0 1
    gt = torch.cat([c["gt_gpu"], c["gt_gpu"]])
    assert int(gt[0].max()) == 255
    res = score.score_video(pred, gt, bound_th=c["radius"])
    assert res["n"] == 2 and res["J"].shape == (2, 2)
    want = c["counts"][:, [1, 0]]
    assert np.array_equal(res["counts"], want)
    assert np.array_equal(_bits(res["J"]), _bits(c["J"][:, [1, 0]])) and np.array_equal(_bits(res["F"]), _bits(c["F"][:, [1, 0]]))


# ---------------------------------------------------------------------------------------------------------- the footprint
@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(64 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


def _jf_case(S, T, n, H, W, radius, shift_p, shift_g):
    """Every buffer of the call in the slab; the label planes start `shift` bytes into their buffers (odd base addresses), labels
    0 .. n+1 so that some pixels carry a label above n."""
    total = T * H * W
    rp = S.randint("pred", (shift_p + total + 3,), 0, n + 2, dtype=torch.uint8)
    rg = S.randint("gt", (shift_g + total + 3,), 0, n + 2, dtype=torch.uint8)
    # blocks instead of noise on half of every frame, so boundaries are sparse there and dense elsewhere
    for raw, sh, lab in ((rp, shift_p, 1), (rg, shift_g, n)):
        v = raw[sh:sh + total].view(T, H, W)
        v[:, :, :W // 2] = 0
        v[:, H // 4:H // 2 + sh, W // 8:W // 3] = lab
    counts = S.alloc("counts", (n * T * 6,), dtype=torch.int32)
    ws = S.alloc("ws", (_lib.lib_raw().tce_jf_ws_bytes(T, n, H, W, radius) // 8,), dtype=torch.int64)
    pred, gt = rp.data_ptr() + shift_p, rg.data_ptr() + shift_g

    def fn():
        _lib.check(_lib.lib().tce_jf_counts_i32(pred, gt, counts.data_ptr(), ws.data_ptr(), T, n, H, W, radius,
                                                torch.cuda.current_stream().cuda_stream), "tce_jf_counts_i32")
    fn.check = lambda: (rp[shift_p:shift_p + total].view(T, H, W), rg[shift_g:shift_g + total].view(T, H, W), counts)
    return fn


FOOTPRINT_CASES = [
    ("two_frames_3_objects_70x131_radius_3_addresses_1_and_3", dict(T=2, n=3, H=70, W=131, radius=3, shift_p=1, shift_g=3)),
    ("one_frame_2_objects_7x9_radius_1_address_3_and_1", dict(T=1, n=2, H=7, W=9, radius=1, shift_p=3, shift_g=1)),
]


@pytest.mark.parametrize("tag,kw", FOOTPRINT_CASES, ids=[c[0] for c in FOOTPRINT_CASES])
def test_jf_counts_footprint(slab, tag, kw):
    """W, O and R of tests/_footprint.py, no exemptions: nothing outside counts and ws is written, every word of counts (and of ws)
    is written, and the result depends on no byte outside pred, gt -- the bytes around the oddly placed planes included -- and on
    nothing ws held before the call (ws is scratch: R fills it before the run)."""
    info = fp.check_case(slab, lambda S: _jf_case(S, **kw), fp.recorder("tce_jf_counts_i32"), scratch=("ws",), props="WOR", sync=torch.cuda.synchronize, label=tag)
    print(f"{tag}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']} untouched-in-buffers {info['pad_bytes']}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == []
    T, n, H, W = kw["T"], kw["n"], kw["H"], kw["W"]
    wsb = n * T * -(-H // 32) * -(-W // 64) * 24
    assert info["read_bytes"] == 2 * T * H * W + wsb and info["written_bytes"] == n * T * 24 + wsb
    slab.begin(0)
    fn = _jf_case(slab, **kw)
    fn()
    torch.cuda.synchronize()
    pred, gt, counts = fn.check()
    want, _, _ = _jf.reference(pred.cpu().numpy(), gt.cpu().numpy(), n, kw["radius"])
    _assert_counts(counts.view(n, T, 6), want, tag)


# ------------------------------------------------------------------------------------------------------------- rejections
def test_rejections():
    from tce_rvos_amd import ops
    u8 = torch.zeros(2, 8, 10, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        ops.jf_counts(u8[..., ::2], u8[..., ::2], 1, 1)
    with pytest.raises(ValueError, match="on the GPU"):
        ops.jf_counts(u8.cpu(), u8, 1, 1)
    with pytest.raises(ValueError, match="same shape"):
        ops.jf_counts(u8, u8[:1], 1, 1)
    with pytest.raises(ValueError, match="uint8"):
        ops.jf_counts(u8, u8.float(), 1, 1)
    for n, radius in ((0, 1), (17, 1), (1, -1), (1, 41)):
        with pytest.raises(ValueError, match="unsupported"):
            ops.jf_counts(u8, u8, n, radius)
    with pytest.raises(ValueError, match="counts"):
        ops.jf_counts(u8, u8, 1, 1, counts=torch.zeros(1, 2, 5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="ws"):
        ops.jf_counts(u8, u8, 1, 1, ws=torch.zeros(1, dtype=torch.int64, device="cuda"))
    out = ops.jf_counts(u8, u8, 2, 1)  # all background: nothing anywhere
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 2, 6) and not bool(out.any())
    # the C entry itself, on real buffers
    l = _lib.lib()
    cnt = torch.full((2 * 2 * 6,), 7, dtype=torch.int32, device="cuda")
    ws = torch.full((2 * 2 * 3 + 1,), 7, dtype=torch.int64, device="cuda")
    p, c, w = u8.data_ptr(), cnt.data_ptr(), ws.data_ptr()
    assert l.tce_jf_counts_i32(None, p, c, w, 2, 2, 8, 10, 1, None) != 0 and b"tce_jf_counts_i32" in l.tce_last_error()
    assert l.tce_jf_counts_i32(p, None, c, w, 2, 2, 8, 10, 1, None) != 0
    assert l.tce_jf_counts_i32(p, p, None, w, 2, 2, 8, 10, 1, None) != 0
    assert l.tce_jf_counts_i32(p, p, c, None, 2, 2, 8, 10, 1, None) != 0
    assert l.tce_jf_counts_i32(p, p, c, w, 2, 0, 8, 10, 1, None) != 0 and b"objects" in l.tce_last_error()
    assert l.tce_jf_counts_i32(p, p, c, w, 2, 17, 8, 10, 1, None) != 0
    assert l.tce_jf_counts_i32(p, p, c, w, 2, 2, 8, 10, -1, None) != 0 and b"radius" in l.tce_last_error()
    assert l.tce_jf_counts_i32(p, p, c, w, 2, 2, 8, 10, 41, None) != 0
    assert l.tce_jf_counts_i32(p, p, c, w, 2, 2, 0, 10, 1, None) != 0 and b"extent" in l.tce_last_error()
    assert l.tce_jf_counts_i32(p, p, c, w + 4, 2, 2, 8, 10, 1, None) != 0 and b"aligned" in l.tce_last_error()
    torch.cuda.synchronize()
    assert bool((cnt == 7).all()) and bool((ws == 7).all())  # a rejected call launches nothing
