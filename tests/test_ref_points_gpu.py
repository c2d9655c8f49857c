"""GPU: the opt-in ref_points=True of video.run_video / run_video_expressions -- reference_points [N,2] are the best query's rows of
the forward's reference_points, gathered like pred_boxes; without the flag the dicts are what they were; the result draws through
vis.overlay_expression."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, N = 32, 48, 5
CAPTIONS = ["a kite", "the red kite that flies over the beach"]
KEYS = {"masks", "best_query", "pred_logits", "pred_boxes"}


def _same(a, b):
    """two runs of one program: integers equal, floats to 1e-5 (sigmoid outputs and logits of order 1; a wrong query's rows differ
    in the first digits)"""
    return torch.equal(a, b) if not a.is_floating_point() else torch.allclose(a, b, rtol=0, atol=1e-5)


@pytest.fixture(scope="module")
def model():
    from tce_rvos_amd import build_model, load_synth_weights
    args = argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)
    m, _, _ = build_model(args)
    m = m.cuda().eval()
    load_synth_weights(m, 37)
    m.repack()
    return m


@pytest.fixture(scope="module")
def frames():
    return torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(2)).cuda()


def test_run_video_returns_the_best_query_s_reference_points(model, frames):
    from tce_rvos_amd import video, vis
    plain = video.run_video(model, frames, CAPTIONS[1], (40, 60), clip_size=3)
    res = video.run_video(model, frames, CAPTIONS[1], (40, 60), clip_size=3, ref_points=True)
    assert set(plain) == KEYS and set(res) == KEYS | {"reference_points"}
    for k in KEYS:
        assert _same(plain[k], res[k]), k
    pts = res["reference_points"]
    assert tuple(pts.shape) == (N, 2) and pts.dtype == torch.float32
    want = []
    for c, lo in enumerate(range(0, N, 3)):  # the forward's own rows, chunk by chunk
        out = model([frames[lo:lo + 3]], [CAPTIONS[1]], [{"size": torch.tensor([H, W])}])
        q = int(res["best_query"][c])
        want.append(out["reference_points"][0][:, q])
        assert _same(out["pred_boxes"][0][:, q], res["pred_boxes"][lo:lo + 3])
    assert _same(torch.cat(want, 0), pts)
    u8 = torch.randint(0, 256, (N, 40, 60, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    img = vis.overlay_expression(u8, res, [255, 0, 0])
    assert tuple(img.shape) == (N, 40, 60, 3) and not torch.equal(img, u8)
    assert not torch.equal(img, vis.overlay_expression(u8, plain, [255, 0, 0]))      # the cross is what ref_points adds


def test_run_video_expressions_returns_them_per_caption(model, frames):
    from tce_rvos_amd import video
    plain = video.run_video_expressions(model, frames, CAPTIONS, (40, 60), clip_size=3, mixed_lengths=True)
    res = video.run_video_expressions(model, frames, CAPTIONS, (40, 60), clip_size=3, mixed_lengths=True, ref_points=True)
    for p, r in zip(plain, res):
        assert set(p) == KEYS and set(r) == KEYS | {"reference_points"}
        for k in KEYS:
            assert _same(p[k], r[k]), k
        assert tuple(r["reference_points"].shape) == (N, 2)
    alone = video.run_video(model, frames, CAPTIONS[0], (40, 60), clip_size=3, ref_points=True)
    if torch.equal(alone["best_query"], res[0]["best_query"]):  # the same queries: the same points, to the round-off between group shapes
        assert torch.allclose(alone["reference_points"], res[0]["reference_points"], rtol=0, atol=1e-3)
