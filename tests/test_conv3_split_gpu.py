"""GPU: the 3x3 convolution's split form (tce_conv3x3_split_f32): a launch that fills less than one round of workgroups walks the
K dimension in pieces, and a reduce pass adds the fp32 partials in piece order and the bias."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tce_rvos_amd import ops as _ops
    return _ops


@pytest.fixture
def lib():
    from tce_rvos_amd._lib import lib as _lib
    yield _lib()
    _lib().tce_debug_conv3x3_set_pieces(0)
    _lib().tce_debug_conv3x3_set_waves(0)


def _problem(T, H, W, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(T * H * W, 256, generator=g).cuda()
    w = torch.randn(256, 256, 3, 3, generator=g) / 48.0
    b = torch.randn(256, generator=g).cuda()
    w_cl = w.permute(0, 2, 3, 1).reshape(256, -1).contiguous().cuda()
    x64 = x.view(T, H, W, 256).permute(0, 3, 1, 2).double()
    ref = torch.nn.functional.conv2d(x64, w.cuda().double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(T * H * W, 256)
    return x, w_cl, b, ref


def _split(lib, x, pk, b, out, T, H, W, ws):
    nws = int(lib.tce_conv3x3_split_ws_floats(T * H * W, 256, 256))
    assert ws.numel() >= nws
    rc = lib.tce_conv3x3_split_f32(x.data_ptr(), x.stride(0), pk.data_ptr(), b.data_ptr(), out.data_ptr(), out.stride(0), T, H, W,
                                   256, 256, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.tce_last_error()
    return nws


def _evict_caches():
    junk = torch.empty(768 << 20, dtype=torch.uint8, device="cuda")
    junk.fill_(1)
    torch.cuda.synchronize()
    del junk


# 72000 / 18000 px: config 2's stride-4 (mixed form: split remainder) and stride-8 (single sub-round launch) maps; 128400 / 122880:
# larger maps (nothing split); odd sizes whose pieces' blocks straddle frame boundaries and image edges.  pieces 0 = the plan's own.
@pytest.mark.parametrize("T,H,W", [(5, 90, 160), (5, 45, 80), (10, 120, 107), (8, 96, 160), (3, 37, 113), (1, 257, 256), (2, 131, 67)])
@pytest.mark.parametrize("pieces,waves", [(0, 0), (5, 0), (0, 4), (2, 4)])
def test_split_against_unsplit_and_fp64(ops, lib, T, H, W, pieces, waves):
    M = T * H * W
    x, w_cl, b, ref = _problem(T, H, W, seed=M % 1000 + pieces)
    pk = ops.conv3x3_pack(w_cl, 256)
    lib.tce_debug_conv3x3_set_waves(waves)
    lib.tce_debug_conv3x3_set_pieces(pieces)
    base = ops.conv3x3(x, pk, T, H, W, 256, 256, bias=b)           # no allocator: tce_conv3x3_f32
    ws = torch.full((max(1, int(lib.tce_conv3x3_split_ws_floats(M, 256, 256))),), float("nan"), device="cuda")
    out = torch.full((M, 256), float("nan"), device="cuda")
    _evict_caches()
    _split(lib, x, pk, b, out, T, H, W, ws)
    torch.cuda.synchronize()
    scale = ref.abs().max().item()
    err = (out.double() - ref).abs().amax(dim=1)
    bad = int((~(err < 2e-5 * scale)).sum())
    assert bad == 0, f"{bad} of {M} pixels wrong against fp64 (max err {err.nan_to_num(1e30).max().item():.3e}, scale {scale:.3e})"
    assert (out - base).abs().max().item() < 2e-5 * scale
    if lib.tce_conv3x3_split_pieces(M, 256, 256) == 1:
        assert torch.equal(out, base)  # nothing split: the launches of tce_conv3x3_f32


def test_split_workspace_reused_by_another_shape(ops, lib):
    """One workspace, three launches A, B, A: B's partials left in it do not leak into A's second result."""
    shapes = ((5, 45, 80), (3, 37, 113))
    probs = [_problem(*s, seed=3 + i) for i, s in enumerate(shapes)]
    pk = [ops.conv3x3_pack(p[1], 256) for p in probs]
    nws = max(int(lib.tce_conv3x3_split_ws_floats(T * H * W, 256, 256)) for (T, H, W) in shapes)
    assert nws > 0
    ws = torch.empty(nws, device="cuda")
    outs = [torch.empty(T * H * W, 256, device="cuda") for (T, H, W) in shapes] + [None]
    outs[2] = torch.empty_like(outs[0])
    for i, k in enumerate((0, 1, 0)):
        x, _, b, _ = probs[k]
        _split(lib, x, pk[k], b, outs[i], *shapes[k], ws)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[2])
    for i, k in enumerate((0, 1)):
        ref = probs[k][3]
        assert (outs[i].double() - ref).abs().max().item() < 2e-5 * ref.abs().max().item()


@pytest.mark.parametrize("T,H,W", [(5, 90, 160), (5, 45, 80)])
def test_split_replay_equals_eager_bitwise(ops, lib, T, H, W):
    """Pieces are summed in piece order whatever order they ran in: eager runs and a captured graph's replays are bit-identical."""
    M = T * H * W
    x, w_cl, b, _ = _problem(T, H, W, seed=21)
    pk = ops.conv3x3_pack(w_cl, 256)
    assert lib.tce_conv3x3_split_pieces(M, 256, 256) > 1
    ws = torch.empty(int(lib.tce_conv3x3_split_ws_floats(M, 256, 256)), device="cuda")
    eager = [torch.empty(M, 256, device="cuda") for _ in range(2)]
    for o in eager:
        _split(lib, x, pk, b, o, T, H, W, ws)
    torch.cuda.synchronize()
    assert torch.equal(eager[0], eager[1])
    rep = torch.empty(M, 256, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _split(lib, x, pk, b, rep, T, H, W, ws)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _split(lib, x, pk, b, rep, T, H, W, ws)
    for _ in range(3):
        rep.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rep, eager[0])
    del graph
