"""The rules the output stages share (csrc/mask_planes.h), held as exact equalities between the entry points that use them: the
mask-resampling rule and the best-query score of tce_select_masks_u8, tce_label_objects_u8 and tce_a2d_masks_u8 give the same bits
(no contested-pixel allowance), and the byte-quad rule writes exactly its plane at the smallest planes and every start address."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("t", [0.3, 0.5])
def test_label_map_of_one_object_equals_the_harness_mask(t):
    """With background == threshold both rules reduce to s > t: a score below t becomes 0, and a score equal to t ties with the
    background plane, which wins as the first maximum.  Odd sizes; the 1026 label bytes start and end mid-dword; 19/5 and 27/7 give
    non-dyadic weights."""
    from tce_rvos_amd import ops
    T, Q, K, h, w, size = 2, 3, 1, 5, 7, (19, 27)
    g = torch.Generator().manual_seed(12)
    lg = torch.randn(T, Q, K, generator=g).cuda()
    pm = (torch.randn(T, Q, h, w, generator=g) * 3).cuda()
    want, want_best = ops.select_masks(lg, pm, size, threshold=t)
    flat = torch.empty(1 + T * size[0] * size[1], dtype=torch.uint8, device="cuda")
    got, got_best = ops.label_objects([lg], [pm], size, threshold=t, background=t, out=flat[1:].view(T, *size))
    torch.cuda.synchronize()
    assert got.data_ptr() % 4 == 1
    assert 0 < int(want.sum()) < want.numel()
    assert torch.equal(got_best, want_best)
    assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("t", [0.3, 0.5])
def test_a2d_mask_at_the_model_size_equals_the_harness_mask(t):
    """H0 == fh: the nearest index is the identity (floorf(yo * 1.0f)), and (float)h / (float)(4h) is exactly 0.25f, so the two kernels
    evaluate the same taps."""
    from tce_rvos_amd import ops
    N, h, w = 3, 5, 7
    size = (4 * h, 4 * w)
    g = torch.Generator().manual_seed(13)
    pm = (torch.randn(N, h, w, generator=g) * 3).cuda()
    lg = torch.randn(N, 1, 1, generator=g).cuda()
    want, _ = ops.select_masks(lg, pm[:, None].contiguous(), size, threshold=t)
    got = ops.a2d_masks(pm, size, size, threshold=t)
    torch.cuda.synchronize()
    assert 0 < int(want.sum()) < want.numel()
    assert torch.equal(got, want), int((got != want).sum())


def _label_objects(size, out):
    from tce_rvos_amd import ops
    g = torch.Generator().manual_seed(14)
    lg = [torch.randn(1, 2, 1, generator=g).cuda() for _ in range(2)]
    pm = [(torch.randn(1, 2, 2, 3, generator=g) * 3).cuda() for _ in range(2)]
    return ops.label_objects(lg, pm, size, out=out)[0]


def _a2d_masks(size, out):
    from tce_rvos_amd import ops
    pm = (torch.randn(1, 2, 3, generator=torch.Generator().manual_seed(15)) * 3).cuda()
    return ops.a2d_masks(pm, (8, 12), size, out=out)


@pytest.mark.parametrize("size", [(1, 1), (1, 3), (2, 3), (3, 5)])
@pytest.mark.parametrize("op", [_label_objects, _a2d_masks])
def test_byte_quads_at_the_smallest_planes_and_every_start_address(op, size):
    """One plane of 1, 3, 6 and 15 bytes (less than a dword; a dword and a half; head, whole dwords and tail) at each address mod 4:
    the call's own allocation and the slice agree, and the bytes on both sides of the slice are left alone."""
    total = size[0] * size[1]
    own = op(size, None)
    torch.cuda.synchronize()
    assert tuple(own.shape) == (1,) + size and own.data_ptr() % 4 == 0
    for shift in range(4):
        flat = torch.full((8 + total + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        lo = 4 + shift
        out = flat[lo:lo + total].view(1, *size)
        assert out.data_ptr() % 4 == shift
        got = op(size, out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and torch.equal(out, own), (shift, out.tolist(), own.tolist())
        assert bool((flat[:lo] == 0xEE).all()) and bool((flat[lo + total:] == 0xEE).all()), (shift, flat.tolist())
