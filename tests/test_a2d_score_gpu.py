"""A2D-Sentences / JHMDB-Sentences scoring on the GPU: tce_rle_decode_u8 and tce_mask_overlap_i32 (include/tce_rvos_score.h)
against numpy (tests/_a2d.py: rle_decode is the yardstick; the contract's own formula for counts that are no mask's run lengths),
their access models against the bytes the launches touch (tests/_footprint.py), and a2d_score.A2DScorer end to end against the fixture of the reference's own function (tests/golden/a2d_score_cases.npz) and the
plain-loop restatement of COCOeval (tests/_a2d_score.py; not pycocotools)."""
import os

import numpy as np
import pytest
import torch

import _a2d
import _a2d_score as S
import _footprint as fp
from tce_rvos_amd import _lib, hazard

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1), (1, 7), (7, 1), (37, 53), (40, 30), (96, 130)]   # (37, 53): odd, no multiple of 4, more positions than one segment
AP_KEYS = ("mAP 0.5:0.95", "AP 0.5", "AP 0.75", "AP 0.5:0.95 S", "AP 0.5:0.95 M", "AP 0.5:0.95 L")


# ------------------------------------------------------------------------------------------------------------- helpers
def _blob_masks(H, W, seed):
    """five masks [5,H,W]: all zero (one run), all one (first count 0), a single 1 at the first pixel, a blob, noise"""
    rng = np.random.default_rng(seed)
    first = np.zeros((H, W), np.uint8)
    first[0, 0] = 1
    return np.stack([np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8), first, S._blob(rng, H, W), (rng.random((H, W)) < 0.4).astype(np.uint8)])


def _pack(rows, stride):
    """lists of run lengths -> (counts int32 [P,stride] holding uint32 values, nruns int32 [P]) on the GPU"""
    buf = np.zeros((len(rows), stride), dtype=np.uint32)
    for p, r in enumerate(rows):
        buf[p, :len(r)] = r
    return torch.from_numpy(buf.view(np.int32)).cuda(), torch.tensor([len(r) for r in rows], dtype=torch.int32).cuda()


def _contract(rows, nruns, stride, H, W):
    """the contract of the header, literally: m = clamp(nruns, 0, stride), e_i = min(c_0 + .. + c_i, H*W) in exact integers,
    i(q) = #{i < m: e_i <= q}, out[y,x] = i(q) & 1 if i(q) < m else 0 at q = x*H + y"""
    out = np.zeros((len(rows), H, W), np.uint8)
    for p, r in enumerate(rows):
        c = (list(r) + [0] * stride)[:stride]
        m = min(max(int(nruns[p]), 0), stride)
        e, tot = [], 0
        for i in range(m):
            tot += int(c[i])
            e.append(min(tot, H * W))
        for x in range(W):
            for y in range(H):
                i = sum(1 for v in e if v <= x * H + y)
                out[p, y, x] = (i & 1) if i < m else 0
    return out


def _decode(masks):
    """ops.rle_decode of the loop's run lengths of masks [P,H,W] at stride H*W + 1 -> uint8 [P,H,W] on the host"""
    from tce_rvos_amd import ops
    P, H, W = masks.shape
    rows = [_a2d.rle_counts(m) for m in masks]
    counts, nruns = _pack(rows, H * W + 1)
    got = ops.rle_decode(counts, nruns, (H, W))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (P, H, W)
    want = np.stack([_a2d.rle_decode(r, H, W) for r in rows])
    assert np.array_equal(want, masks)
    return got.cpu().numpy(), want


# ---------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("H,W", SHAPES)
def test_decode_five_masks_in_one_call(H, W):
    got, want = _decode(_blob_masks(H, W, 7))
    for p in range(5):
        assert np.array_equal(got[p], want[p]), (H, W, p, int((got[p] != want[p]).sum()))


@pytest.mark.parametrize("H,W", SHAPES)
def test_decode_one_mask_per_call(H, W):
    for p, m in enumerate(_blob_masks(H, W, 8)):
        got, want = _decode(m[None])
        assert np.array_equal(got, want), (H, W, p)


@pytest.mark.parametrize("P", [1, 5])
def test_decode_checkerboard_of_h_w_plus_one_runs(P):
    """40 x 30 = 1200 positions; the column-major checkerboard that starts with a 1 has 1201 runs (the first count is 0): past one
    segment of 1024 counts"""
    H, W = 40, 30
    cols = [((np.arange(H * W) + k) & 1).astype(np.uint8) for k in (1, 0, 1, 0, 1)][:P]
    masks = np.stack([np.ascontiguousarray(c.reshape(W, H).T) for c in cols])
    assert len(_a2d.rle_counts(masks[0])) == H * W + 1
    got, want = _decode(masks)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("H,W,P,off", [(37, 53, 5, 1), (37, 53, 5, 2), (37, 53, 5, 3), (7, 1, 1, 1), (1, 7, 5, 3), (1, 1, 1, 2)])
def test_decode_into_an_unaligned_slice_leaves_its_neighbours_alone(H, W, P, off):
    """37 * 53 = 1961 is odd, so the five planes of one call start at five different addresses mod 4"""
    from tce_rvos_amd import ops
    masks = _blob_masks(H, W, 9)[-P:]
    counts, nruns = _pack([_a2d.rle_counts(m) for m in masks], H * W + 1)
    n = P * H * W
    flat = torch.full((off + n + 9,), 0xAA, dtype=torch.uint8, device="cuda")
    out = flat[off:off + n].view(P, H, W)
    assert out.data_ptr() % 4 == off
    got = ops.rle_decode(counts, nruns, (H, W), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = flat.cpu().numpy()
    assert (host[:off] == 0xAA).all() and (host[off + n:] == 0xAA).all()
    assert host[off:off + n].max() <= 1 and np.array_equal(host[off:off + n].reshape(P, H, W), masks)


def test_decode_does_not_depend_on_the_workspace_and_repeats():
    from tce_rvos_amd import _lib, ops
    H, W, P = 37, 53, 5
    masks = _blob_masks(H, W, 10)
    counts, nruns = _pack([_a2d.rle_counts(m) for m in masks], H * W + 1)
    nbytes = _lib.lib().tce_rle_decode_ws_bytes(P, H, W, H * W + 1)
    assert nbytes >= (P * (H * W + 1) + P * 2) * 4 and nbytes % 8 == 0
    outs = []
    for fill in (0x00, 0xFF, 0xFF):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        outs.append(ops.rle_decode(counts, nruns, (H, W), ws=ws).clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2]) and np.array_equal(outs[0].cpu().numpy(), masks)
    with pytest.raises(ValueError, match="ws must hold"):
        ops.rle_decode(counts, nruns, (H, W), ws=torch.zeros(nbytes // 8 - 1, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("H,W", [(37, 53), (96, 130), (1, 7)])
def test_decode_of_the_encoders_counts_is_the_mask(H, W):
    """decode(rle_counts(m)) == m, on the device with no read-back in between: the encoder's layout is the decoder's"""
    from tce_rvos_amd import ops
    m = torch.from_numpy(_blob_masks(H, W, 11)).cuda()
    m[3] *= 7                                             # the encoder takes any nonzero byte as set; the decoder writes 1
    counts, nruns = ops.rle_counts(m)
    back = ops.rle_decode(counts, nruns, (H, W))
    torch.cuda.synchronize()
    assert torch.equal(back, (m != 0).to(torch.uint8))


HAND = [
    # name, (H, W), stride, rows, nruns (None: the rows' lengths)
    ("zero-length runs in the middle flip parity", (3, 4), 9, [[2, 0, 3, 0, 0, 4, 3]], None),
    ("short of the plane: the tail is 0", (3, 4), 5, [[1, 2, 1, 3], [0, 5]], None),
    ("past the plane: clipped", (3, 4), 4, [[4, 100], [0, 7, 2, 900], [13]], None),
    ("sums past 32 bits do not wrap", (5, 3), 6, [[3, 0xFFFFFFFF, 0xFFFFFFFF, 5], [0xFFFFFFFF, 1], [0, 0x80000000, 0x80000000, 2]], None),
    ("nruns 0, negative, beyond the stride, and short of the row", (3, 4), 4, [[2, 3, 4, 3]] * 4, [0, -5, 9, 2]),
    ("a stride of one", (2, 2), 1, [[3], [0]], [1, 1]),
    ("counts in the third segment, stride no multiple of it", (6, 7), 2100, [[0] * 2049 + [5, 1, 30, 6], [1] * 42, [0] * 1024 + [20, 22]], None),
]


@pytest.mark.parametrize("name,hw,stride,rows,nruns", HAND, ids=[c[0] for c in HAND])
def test_decode_hand_made_counts(name, hw, stride, rows, nruns):
    from tce_rvos_amd import ops
    H, W = hw
    counts, nr = _pack(rows, stride)
    if nruns is not None:
        nr = torch.tensor(nruns, dtype=torch.int32).cuda()
    nruns = nr.cpu().tolist()
    got = ops.rle_decode(counts, nr, hw)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = _contract(rows, nruns, stride, H, W)
    print(name, got.reshape(len(rows), -1).tolist())
    assert np.array_equal(got, want), name
    col = got.transpose(0, 2, 1).reshape(len(rows), -1)   # the column-major walk
    if name.startswith("zero-length"):
        assert col[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0]      # 2 zeros | 0 ones | 3 zeros | 0 | 0 | 4 ones | 3 zeros
    if name.startswith("short"):
        assert col[0].tolist() == [0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 0] and col[1].tolist() == [1] * 5 + [0] * 7
    if name.startswith("past"):
        assert col[0].tolist() == [0] * 4 + [1] * 8 and col[1].tolist() == [1] * 7 + [0] * 2 + [1] * 3 and not col[2].any()
    if name.startswith("sums"):
        assert col[0].tolist() == [0] * 3 + [1] * 12 and not col[1].any() and col[2].tolist() == [1] * 15
    if name.startswith("nruns"):
        assert not col[0].any() and not col[1].any() and col[2].tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1]
        assert col[3].tolist() == [0, 0, 1, 1, 1] + [0] * 7


def test_decode_rejections():
    from tce_rvos_amd import ops
    counts, nruns = _pack([[12]], 13)
    with pytest.raises(ValueError, match="int32"):
        ops.rle_decode(counts.to(torch.int64), nruns, (3, 4))
    with pytest.raises(ValueError, match="on the GPU"):
        ops.rle_decode(counts.cpu(), nruns, (3, 4))
    with pytest.raises(ValueError, match="contiguous"):
        ops.rle_decode(torch.zeros(1, 26, dtype=torch.int32, device="cuda")[:, ::2], nruns, (3, 4))
    with pytest.raises(ValueError, match="agree in P"):
        ops.rle_decode(counts, torch.zeros(2, dtype=torch.int32, device="cuda"), (3, 4))
    with pytest.raises(ValueError, match="unsupported extents"):
        ops.rle_decode(counts, nruns, (0, 4))
    with pytest.raises(ValueError, match="unsupported extents"):
        ops.rle_decode(counts, nruns, (1 << 16, 1 << 15))
    with pytest.raises(ValueError, match="out"):
        ops.rle_decode(counts, nruns, (3, 4), out=torch.empty(1, 4, 3, dtype=torch.uint8, device="cuda"))


# --------------------------------------------------------------------------------------------------------------- overlap
def _planes(N, H, W, seed):
    """pred [N,H,W] and gt [H,W] with bytes other than 0 / 1; with N = 5, pred[0] is empty, pred[1] has gt's support"""
    rng = np.random.default_rng(seed)
    vals = np.array([0, 0, 0, 1, 1, 2, 128, 255], np.uint8)
    pred = vals[rng.integers(0, len(vals), (N, H, W))]
    gt = vals[rng.integers(0, len(vals), (H, W))]
    if N == 5:
        pred[0] = 0
        pred[1] = (gt != 0) * 3
    return pred, gt


def _at_odd_addresses(pred, gt):
    """the planes copied to addresses 1 and 3 mod 4 of larger GPU buffers"""
    fp = torch.zeros(pred.size + 8, dtype=torch.uint8, device="cuda")
    fg = torch.zeros(gt.size + 8, dtype=torch.uint8, device="cuda")
    p, g = fp[1:1 + pred.size].view(*pred.shape), fg[3:3 + gt.size].view(*gt.shape)
    p.copy_(torch.from_numpy(pred))
    g.copy_(torch.from_numpy(gt))
    assert p.data_ptr() % 4 == 1 and g.data_ptr() % 4 == 3
    return p, g


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("H,W", SHAPES + [(240, 320)])
def test_overlap_counts_equal_numpy(H, W, N):
    """240 x 320 with N = 5 is the dataset's own plane: 75 tiles"""
    from tce_rvos_amd import ops
    pred, gt = _planes(N, H, W, 31 + N)
    p, g = _at_odd_addresses(pred, gt)
    slab = torch.full((4, N, 3), -77, dtype=torch.int32, device="cuda")
    got = ops.mask_overlap(p, g, counts=slab[2])
    torch.cuda.synchronize()
    assert got.data_ptr() == slab[2].data_ptr()
    host = slab.cpu().numpy()
    want = S.overlap_counts(pred, gt)
    print(f"{N} x {H} x {W}: {host[2].tolist()}")
    assert np.array_equal(host[2], want)
    assert (host[[0, 1, 3]] == -77).all()
    if N == 5:
        assert host[2, 0, :2].tolist() == [0, 0] and host[2, 1, 0] == host[2, 1, 1] == host[2, 1, 2]


def test_overlap_empty_ground_truth_and_aligned_planes():
    from tce_rvos_amd import ops
    pred, _ = _planes(5, 37, 53, 40)
    got = ops.mask_overlap(torch.from_numpy(pred).cuda(), torch.zeros(37, 53, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and tuple(got.shape) == (5, 3)
    assert np.array_equal(got.cpu().numpy(), S.overlap_counts(pred, np.zeros((37, 53), np.uint8)))
    assert not got[:, 0].any() and not got[:, 2].any() and bool(got[2:, 1].all())


def test_overlap_does_not_depend_on_the_workspace_and_repeats():
    from tce_rvos_amd import _lib, ops
    N, H, W = 5, 96, 130
    pred, gt = _planes(N, H, W, 41)
    p, g = _at_odd_addresses(pred, gt)
    nbytes = _lib.lib().tce_mask_overlap_ws_bytes(N, H, W)
    tiles = -(-H * W // 1024)
    assert nbytes == ((N * tiles * 2 + tiles) * 4 + 7) // 8 * 8
    outs = []
    for fill in (0x00, 0xFF, 0xFF):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        outs.append(ops.mask_overlap(p, g, ws=ws).clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    assert np.array_equal(outs[0].cpu().numpy(), S.overlap_counts(pred, gt))


def test_overlap_rejections():
    from tce_rvos_amd import ops
    p, g = torch.zeros(2, 4, 6, dtype=torch.uint8, device="cuda"), torch.zeros(4, 6, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="uint8"):
        ops.mask_overlap(p.float(), g)
    with pytest.raises(ValueError, match="on the GPU"):
        ops.mask_overlap(p, g.cpu())
    with pytest.raises(ValueError, match="contiguous"):
        ops.mask_overlap(torch.zeros(2, 4, 12, dtype=torch.uint8, device="cuda")[..., ::2], g)
    with pytest.raises(ValueError, match="same plane"):
        ops.mask_overlap(p, torch.zeros(6, 4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="counts"):
        ops.mask_overlap(p, g, counts=torch.zeros(2, 3, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="counts"):
        ops.mask_overlap(p, g, counts=torch.zeros(2, 6, dtype=torch.int32, device="cuda")[:, ::2])


# --------------------------------------------------------------------------------------------- the recorder and the footprint
def test_hazard_recording_lists_the_one_entry_of_each_wrapper():
    from tce_rvos_amd import ops
    H, W = 37, 53
    masks = _blob_masks(H, W, 12)
    counts, nruns = _pack([_a2d.rle_counts(m) for m in masks], H * W + 1)
    pred, gt = _at_odd_addresses(*_planes(5, H, W, 43))
    want = ops.rle_decode(counts, nruns, (H, W)), ops.mask_overlap(pred, gt)
    with hazard.recording() as rec:
        planes = ops.rle_decode(counts, nruns, (H, W))
    with hazard.recording() as rec2:
        overlap = ops.mask_overlap(pred, gt)
    torch.cuda.synchronize()
    assert [x.name for x in rec.launches] == ["tce_rle_decode_u8"] and [x.name for x in rec2.launches] == ["tce_mask_overlap_i32"]
    assert rec.analyse().clean and rec2.analyse().clean
    assert torch.equal(planes, want[0]) and torch.equal(overlap, want[1]) and np.array_equal(planes.cpu().numpy(), masks)


@pytest.fixture(scope="module")
def slab():
    s = fp.Slab(64 << 20, device="cuda")
    yield s
    del s
    torch.cuda.empty_cache()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _decode_case(S_, masks, nruns, stride, shift):
    """Every buffer of the call in the slab; out starts `shift` bytes into its buffer.  nruns: None (the rows' own lengths) or the
    values to pass instead."""
    P, H, W = masks.shape
    rows = [_a2d.rle_counts(m) for m in masks]
    buf = np.zeros((P, stride), dtype=np.uint32)
    for p, r in enumerate(rows):
        buf[p, :len(r)] = r
    counts = S_.put("counts", buf.view(np.int32))
    nr = S_.put("nruns", [len(r) for r in rows] if nruns is None else nruns, dtype=torch.int32)
    raw = S_.alloc("out", (shift + P * H * W + 3,), dtype=torch.uint8)
    ws = S_.alloc("ws", (_lib.lib_raw().tce_rle_decode_ws_bytes(P, H, W, stride) // 8,), dtype=torch.int64)
    out = raw.data_ptr() + shift

    def fn():
        _lib.check(_lib.lib().tce_rle_decode_u8(counts.data_ptr(), nr.data_ptr(), out, ws.data_ptr(), P, H, W, stride, _stream()),
                   "tce_rle_decode_u8")
    fn.check = lambda: raw[shift:shift + P * H * W].view(P, H, W)
    return fn


def _decode_footprint_cases():
    rng = np.random.default_rng(51)
    small = (rng.random((3, 5, 7)) < 0.5).astype(np.uint8)
    H, W = 33, 65
    board = np.ascontiguousarray(((np.arange(H * W) + 1) & 1).astype(np.uint8).reshape(W, H).T)[None]  # starts with a 1: H*W + 1 runs
    return [
        # 35-byte planes, so planes 2 and 3 start on odd addresses; the row of plane 1 is not in use at all
        ("three_5x7_planes_stride_36_one_row_unused_address_1", dict(masks=small, nruns="second row 0", stride=36, shift=1)),
        # 2146 runs: more than two segments of 1024 counts
        ("checkerboard_33x65_of_2146_runs_address_3", dict(masks=board, nruns=None, stride=H * W + 1, shift=3)),
    ]


DECODE_FOOTPRINT = _decode_footprint_cases()


@pytest.mark.parametrize("tag,kw", DECODE_FOOTPRINT, ids=[c[0] for c in DECODE_FOOTPRINT])
def test_rle_decode_footprint(slab, tag, kw):
    """W, O and R of tests/_footprint.py: nothing outside out and ws is written (the bytes around the oddly placed planes included),
    every byte of out is written, and the result depends on no byte outside counts and nruns, nor on what ws held (scratch: R fills
    it before the run).  ws is exempt from O: the e_i behind a row's last run in use and the pad to 8 bytes are never written."""
    masks, stride = kw["masks"], kw["stride"]
    P, H, W = masks.shape
    lens = [len(_a2d.rle_counts(m)) for m in masks]
    nruns = None if kw["nruns"] is None else [lens[0], 0] + lens[2:]
    assert max(lens) <= stride and (kw["nruns"] is None or masks[1].any())
    info = fp.check_case(slab, lambda S_: _decode_case(S_, masks, nruns, stride, kw["shift"]), fp.recorder("tce_rle_decode_u8"),
                         exempt=("ws",), scratch=("ws",), props="WOR", sync=torch.cuda.synchronize, label=tag)
    print(f"{tag}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']} untouched-in-buffers {info['pad_bytes']}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == ["ws"]
    wsb = (P * stride + P * -(-stride // 1024)) * 4 + 7 & ~7
    assert info["read_bytes"] == P * stride * 4 + P * 4 + wsb and info["written_bytes"] == P * H * W + wsb
    slab.begin(0)
    fn = _decode_case(slab, masks, nruns, stride, kw["shift"])
    fn()
    torch.cuda.synchronize()
    want = masks.copy()
    if nruns is not None:
        want[1] = 0  # a row with no run in use decodes to zeros
    assert np.array_equal(fn.check().cpu().numpy(), want)


def _overlap_case(S_, N, H, W, shift_p, shift_g, seed):
    pred, gt = _planes(N, H, W, seed)
    hp, hg = np.zeros(shift_p + pred.size + 3, np.uint8), np.zeros(shift_g + gt.size + 3, np.uint8)
    hp[shift_p:shift_p + pred.size], hg[shift_g:shift_g + gt.size] = pred.reshape(-1), gt.reshape(-1)
    rp, rg = S_.put("pred", hp), S_.put("gt", hg)
    counts = S_.alloc("counts", (N * 3,), dtype=torch.int32)
    ws = S_.alloc("ws", (_lib.lib_raw().tce_mask_overlap_ws_bytes(N, H, W) // 8,), dtype=torch.int64)
    p, g = rp.data_ptr() + shift_p, rg.data_ptr() + shift_g

    def fn():
        _lib.check(_lib.lib().tce_mask_overlap_i32(p, g, counts.data_ptr(), ws.data_ptr(), N, H, W, _stream()), "tce_mask_overlap_i32")
    fn.check = lambda: (counts.view(N, 3), S.overlap_counts(pred, gt))
    return fn


OVERLAP_FOOTPRINT = [
    ("three_5x7_planes_one_tile_addresses_1_and_3", dict(N=3, H=5, W=7, shift_p=1, shift_g=3, seed=52)),
    # 2145 bytes: two full tiles of 1024 and a partial one
    ("two_33x65_planes_three_tiles_addresses_2_and_1", dict(N=2, H=33, W=65, shift_p=2, shift_g=1, seed=53)),
]


@pytest.mark.parametrize("tag,kw", OVERLAP_FOOTPRINT, ids=[c[0] for c in OVERLAP_FOOTPRINT])
def test_mask_overlap_footprint(slab, tag, kw):
    """W, O and R: nothing outside counts and ws is written, every word of counts is written, and the result depends on no byte
    outside pred and gt -- the bytes around the oddly placed planes included -- nor on what ws held.  ws is exempt from O for its
    pad alone: both cases have an odd number of partial sums, so the last 4 of its bytes (the pad to 8) are never written."""
    info = fp.check_case(slab, lambda S_: _overlap_case(S_, **kw), fp.recorder("tce_mask_overlap_i32"), exempt=("ws",), scratch=("ws",),
                         props="WOR", sync=torch.cuda.synchronize, label=tag)
    print(f"{tag}: read {info['read_bytes']} written {info['written_bytes']} guard {info['guard_bytes']} untouched-in-buffers {info['pad_bytes']}")
    assert (info["W"], info["O"], info["R"]) == (2, 2, 3) and info["exempt"] == ["ws"]
    N, HW = kw["N"], kw["H"] * kw["W"]
    tiles = -(-HW // 1024)
    wsb = (N * tiles * 2 + tiles) * 4 + 4
    assert info["read_bytes"] == N * HW + HW + wsb and info["written_bytes"] == N * 12 + wsb
    slab.begin(0)
    fn = _overlap_case(slab, **kw)
    fn()
    torch.cuda.synchronize()
    got, want = fn.check()
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------ the scorer
@pytest.fixture(scope="module")
def score_cases():
    return S.load_cases(os.path.join(GOLDEN, "a2d_score_cases.npz"))


@pytest.mark.parametrize("name", ["hand", "random", "single"])
def test_scorer_on_saved_predictions_equals_the_fixture(score_cases, name):
    """update_rle decodes the ground truth and the prediction strings on the GPU: the precisions equal the reference function's
    exactly, its two IoUs within 1e-12, the AP stats the plain-loop restatement's within 1e-12 (not pycocotools: see the helper)"""
    from tce_rvos_amd.a2d_score import A2DScorer
    c = score_cases[name]
    sc = A2DScorer(S.gt_dict(c["images"]))
    preds = S.predictions(c["images"])
    half = len(c["images"]) // 2 * len(c["images"][0]["preds"])
    sc.update_rle(preds[half:])           # in two calls, the later images first: the summary follows the ground truth's order
    sc.update_rle(preds[:half])
    st = sc.state()
    per = S.per_image_of(c["images"])
    by_id = {im["image_id"]: im for im in per}
    for image_id, scores, counts in zip(st["image_ids"], st["scores"], st["counts"]):
        assert counts == by_id[image_id]["counts"] and scores == by_id[image_id]["scores"], image_id
    res = sc.summarize()
    print(name, res)
    assert [res[f"P@{k}"] for k in S.P_AT] == c["precision"].tolist()
    assert abs(res["overall_iou"] - c["overall_iou"]) <= 1e-12 and abs(res["mean_iou"] - c["mean_iou"]) <= 1e-12
    want = S.coco_mask_ap_loops(per)
    assert max(abs(res[k] - w) for k, w in zip(AP_KEYS, want)) <= 1e-12
    with pytest.raises(ValueError, match="scored already"):
        sc.update_rle(preds[:1])


@pytest.fixture(scope="module")
def post_cases():
    return {c["name"]: c for c in _a2d.load_cases(os.path.join(GOLDEN, "a2d_post_cases.npz"))}


def _outputs(c):
    N = c["logits"].shape[0]
    return {"pred_logits": c["logits"].view(1, 1, N, 1).cuda(), "pred_masks": c["masks"][None, None].cuda()}


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_scorer_update_counts_the_post_processors_own_masks(post_cases, name, monkeypatch):
    """update() on what A2DSentencesPostProcess(rle=False) returns, against a ground truth made here: the per-image counts are
    numpy's on the post-processor's own masks; rle=False changes neither scores nor masks; update() reads nothing back (the
    slabs stay on the device, no .cpu() / .item() / .tolist() / synchronize is called), state() reads back once."""
    from tce_rvos_amd.a2d_score import A2DScorer
    from tce_rvos_amd.postprocess import A2DSentencesPostProcess
    c = post_cases[name]
    H0, W0 = c["orig"]
    gt = S._blob(np.random.default_rng(ord(name)), H0, W0)
    orig, size = torch.tensor([c["orig"]]), torch.tensor([c["size"]])
    full = A2DSentencesPostProcess()(_outputs(c), orig, size)
    lean = A2DSentencesPostProcess(rle=False)(_outputs(c), orig, size)
    assert set(full[0]) == {"scores", "masks", "rle_masks"} and set(lean[0]) == {"scores", "masks"}
    assert torch.equal(full[0]["scores"], lean[0]["scores"]) and torch.equal(full[0]["masks"], lean[0]["masks"])
    sc = A2DScorer({5: {"size": [H0, W0], "counts": S.encode(gt)}, 6: {"size": [H0 + 1, W0], "counts": S.encode(np.zeros((H0 + 1, W0), np.uint8))}})
    torch.cuda.synchronize()
    calls = {"cpu": 0, "item": 0, "tolist": 0, "sync": 0}
    real = {"cpu": torch.Tensor.cpu, "item": torch.Tensor.item, "tolist": torch.Tensor.tolist}

    def counting(key):
        def fn(self, *a, **kw):
            calls[key] += 1
            return real[key](self, *a, **kw)
        return fn
    real_sync = torch.cuda.synchronize
    with monkeypatch.context() as mp:
        for key in real:
            mp.setattr(torch.Tensor, key, counting(key))
        mp.setattr(torch.cuda, "synchronize", lambda *a, **kw: (calls.__setitem__("sync", calls["sync"] + 1), real_sync(*a, **kw))[1])
        sc.update([5], lean)
        assert calls == {"cpu": 0, "item": 0, "tolist": 0, "sync": 0}, calls
        assert sc._counts.is_cuda and sc._scores.is_cuda and sc._counts.dtype == torch.int32
        with pytest.raises(ValueError, match="scored already"):
            sc.update([5], lean)
        with pytest.raises(ValueError, match="unknown image_id"):
            sc.update([7], lean)
        with pytest.raises(ValueError, match="ground truth of"):
            sc.update([6], lean)
        assert calls["cpu"] == 0
        st = sc.state()
        assert calls["cpu"] == 1 and calls["sync"] == 0
    masks = lean[0]["masks"][:, 0].cpu().numpy()
    assert st["image_ids"] == [5] and st["counts"][0] == S.overlap_counts(masks, gt).tolist()
    assert st["scores"][0] == lean[0]["scores"].cpu().double().tolist()
    with pytest.raises(ValueError, match="no predictions"):
        sc.summarize()                                       # image 6 was never scored


def test_scorer_slabs_grow_by_doubling_and_keep_their_rows(score_cases):
    from tce_rvos_amd.a2d_score import A2DScorer
    im = score_cases["single"]["images"][0]
    gt = {k: {"size": list(im["size"]), "counts": im["gt"]} for k in range(40)}
    sc = A2DScorer(gt)
    other = S.encode(np.zeros(tuple(im["size"]), np.uint8))
    for k in range(40):
        sc.update_rle([{"image_id": k, "segmentation": {"size": list(im["size"]), "counts": im["preds"][0] if k % 3 else other}, "score": k / 64}])
    assert sc._counts.shape[0] == 64 and sc._scores.shape[0] == 64
    st = sc.state()
    g = S.per_image_of([im])[0]["counts"][0][2]
    assert st["image_ids"] == list(range(40)) and st["scores"] == [[k / 64] for k in range(40)]
    assert st["counts"] == [[[g, g, g] if k % 3 else [0, 0, g]] for k in range(40)]
    assert sc.summarize()["P@0.9"] == 26 / 40
