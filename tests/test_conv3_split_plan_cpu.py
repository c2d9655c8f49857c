"""CPU: the 3x3 convolution's split plan (host-side, no launch): the pieces of a split launch cover the 144 k-steps of the K walk
exactly once, and the workspace size exported through the C ABI is what the plan's pieces write."""
import pytest


@pytest.fixture(scope="module")
def l():
    from tce_rvos_amd import build as b
    b.build(verbose=False)
    from tce_rvos_amd import _lib
    return _lib.lib()


def test_pieces_cover_the_k_walk_once(l):
    for pieces in range(1, 13):
        starts = [l.tce_conv3x3_split_kstep(pieces, s) for s in range(pieces + 1)]
        assert starts[0] == 0 and starts[-1] == 144, (pieces, starts)
        assert all(b > a for a, b in zip(starts, starts[1:])), (pieces, starts)  # no empty piece, no overlap
        assert all(k % 12 == 0 for k in starts)  # whole iterations of the 12-step unrolled body
        covered = [k for a, b in zip(starts, starts[1:]) for k in range(a, b)]
        assert covered == list(range(144))
    assert l.tce_conv3x3_split_kstep(0, 0) == -1 and l.tce_conv3x3_split_kstep(3, 4) == -1 and l.tce_conv3x3_split_kstep(13, 0) == -1


def _narrow_split_pixels(M, cus=256):
    """Pixels of the launch the plan splits: the mixed form's remainder, or the whole map when it is a single narrow launch."""
    full8 = -(-M // 256) // cus
    r4, r8 = -(-(-(-M // 128)) // cus), -(-(-(-M // 256)) // cus)
    rem = M - full8 * 256 * cus
    mixed4 = 7 * full8 + 4 * -(-(-(-rem // 128)) // cus)
    if full8 >= 1 and rem > 0 and mixed4 < 4 * r4 and mixed4 < 7 * r8:
        return rem
    return M


@pytest.mark.parametrize("M", [72000, 18000, 128400, 122880, 144000, 36800, 12000, 65537, 12543, 17554, 65792])
def test_workspace_matches_the_abi(l, M):
    pieces = l.tce_conv3x3_split_pieces(M, 256, 256)
    ws = l.tce_conv3x3_split_ws_floats(M, 256, 256)
    assert 1 <= pieces <= 12
    if pieces == 1:
        assert ws == 0
        return
    px = _narrow_split_pixels(M)
    blocks = -(-px // 128)
    assert blocks < 256 and blocks * pieces <= 2 * 256  # only sub-round launches, at most two rounds of pieces
    assert ws == pieces * px * 256, (M, pieces, ws, px)


def test_config2_maps_are_split(l):
    # the stride-4 map's mixed-form remainder (6464 px, 51 blocks) and the stride-8 map (18000 px, 141 blocks); full-round maps are not
    assert l.tce_conv3x3_split_pieces(72000, 256, 256) > 1
    assert l.tce_conv3x3_split_pieces(18000, 256, 256) >= 1
    assert l.tce_conv3x3_split_pieces(128400, 256, 256) == 1 and l.tce_conv3x3_split_ws_floats(128400, 256, 256) == 0
    assert l.tce_conv3x3_split_ws_floats(18000, 192, 256) == 0 and l.tce_conv3x3_split_ws_floats(0, 256, 256) == 0


def test_forced_pieces_follow_the_debug_switch(l):
    try:
        assert l.tce_debug_conv3x3_set_pieces(3) == 0
        assert l.tce_conv3x3_split_pieces(72000, 256, 256) == 3
        assert l.tce_conv3x3_split_ws_floats(72000, 256, 256) == 3 * 6464 * 256
        assert l.tce_debug_conv3x3_set_pieces(1) == 0
        assert l.tce_conv3x3_split_ws_floats(72000, 256, 256) == 0
        assert l.tce_debug_conv3x3_set_pieces(13) != 0
    finally:
        l.tce_debug_conv3x3_set_pieces(0)
