"""Ragged clip groups: captions of different token length in one forward_group(..., ragged=True).

Kernels against the existing kernels on the un-padded data (bit for bit: same loops, same fma order), RoBERTa against
HuggingFace with an attention mask, and whole groups against each pair's own B = 1 forward on its un-padded caption."""
import argparse
import os

import numpy as np
import pytest
import torch

from _util import synth_frames

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAD = 1
GROUP_KEYS = ("pred_logits", "pred_boxes", "pred_masks", "memory", "reference_points")


def _args(backbone):
    return argparse.Namespace(backbone=backbone, with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(backbone, salt):
        from tce_rvos_amd import build_model, load_synth_weights
        if backbone not in cache:
            m, _, _ = build_model(_args(backbone))
            cache[backbone] = m.cuda().eval()
        m = cache[backbone]
        load_synth_weights(m, salt)
        m.repack()
        return m
    return get


def _alloc(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="cuda")


def _padded_ids(lens, seed, Lmax=None):
    """[G, Lmax] right-padded ids: caption g = <s> + random tokens + </s>, lens[g] tokens in all"""
    Lmax = Lmax or max(lens)
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lens), Lmax), PAD, dtype=torch.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = torch.randint(3, 50000, (n,), generator=g)
        ids[i, 0] = 0
        ids[i, n - 1] = 2
    return ids


# ------------------------------------------------------------------------------------------------------------- kernels
def test_caption_lens_kernel_matches_host_rule_and_reference_table():
    from tce_rvos_amd import ops
    fx = np.load(os.path.join(GOLDEN, "text_pos_ragged.npz"))
    lens = fx["lens"].tolist()
    ids = _padded_ids(lens, 3).cuda()
    got_lens, kmask, pos = ops.caption_lens(ids, PAD, _alloc)
    torch.cuda.synchronize()
    assert got_lens.cpu().tolist() == lens
    assert np.array_equal(kmask.cpu().numpy() != 0, fx["mask"])
    d = float(np.abs(pos.cpu().numpy().reshape(fx["pos"].shape) - fx["pos"]).max())
    assert d < 2e-6, d
    # the rule on odd rows: no pad at all -> Lmax; a leading pad -> 1 (at least one key)
    odd = torch.tensor([[0, 5, 6, 2], [PAD, PAD, PAD, PAD], [0, 2, PAD, PAD]], dtype=torch.int64).cuda()
    l2, m2, _ = ops.caption_lens(odd, PAD, _alloc)
    torch.cuda.synchronize()
    assert l2.cpu().tolist() == [4, 1, 2]
    assert m2.cpu().tolist() == [[0, 0, 0, 0], [0, 1, 1, 1], [0, 0, 1, 1]]


@pytest.mark.parametrize("group,lens", [(32, (32, 20, 11, 7)), (8, (8, 3, 5))])
def test_xattn_pack_lens_matches_plain_pack_on_each_entry(group, lens):
    from tce_rvos_amd import ops
    from tce_rvos_amd._lib import check, lib
    g = torch.Generator().manual_seed(group)
    G, Lmax = len(lens), max(lens)
    k = torch.randn(G, Lmax, 256, generator=g).cuda()
    v = torch.randn(G, Lmax, 256, generator=g).cuda()
    wqT = (0.05 * torch.randn(257, 256, generator=g)).cuda()
    wo = (0.05 * torch.randn(256, 256, generator=g)).cuda()
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    pk = ops.xattn_pack(k, v, wqT, wo, Lmax, _alloc, group=group, batch=G, lens=lt)
    Hd = 8 * group
    W1, b1, W2 = _alloc(G, Hd, 256), _alloc(G, Hd), _alloc(G, 256, Hd)  # the two-launch form's fold
    check(lib().tce_xattn_prepare_lens_f32(k.data_ptr(), v.data_ptr(), wqT.data_ptr(), wo.data_ptr(), W1.data_ptr(), b1.data_ptr(),
                                           W2.data_ptr(), Lmax, group, G, lt.data_ptr(), None), "tce_xattn_prepare_lens_f32")
    for b, n in enumerate(lens):
        kb, vb = k[b, :n].contiguous(), v[b, :n].contiguous()
        ref = ops.xattn_pack(kb, vb, wqT, wo, n, _alloc, group=group, batch=1)
        rW1, rb1, rW2 = _alloc(Hd, 256), _alloc(Hd), _alloc(256, Hd)
        check(lib().tce_xattn_prepare_f32(kb.data_ptr(), vb.data_ptr(), wqT.data_ptr(), wo.data_ptr(), rW1.data_ptr(), rb1.data_ptr(),
                                          rW2.data_ptr(), n, group, 1, None), "tce_xattn_prepare_f32")
        torch.cuda.synchronize()
        assert torch.equal(pk[b], ref[0]), (group, b)
        assert torch.equal(W1[b], rW1) and torch.equal(b1[b], rb1) and torch.equal(W2[b], rW2), (group, b)


@pytest.mark.parametrize("splits", [1, 3])
def test_mha_small_lens_matches_plain_kernel_on_each_sequence(splits):
    from tce_rvos_amd._lib import check, lib
    lens, H = (9, 4, 17, 1), 12
    G, Lmax, E = len(lens), max(lens), 12 * 64
    g = torch.Generator().manual_seed(splits)
    planes = torch.randn(splits, G * Lmax, 3 * E, generator=g).cuda()
    bias = torch.randn(3 * E, generator=g).cuda() if splits > 1 else None
    bp = bias.data_ptr() if bias is not None else None
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    out = _alloc(G * Lmax, E)
    check(lib().tce_mha_small64_lens_f32(planes.data_ptr(), splits, bp, out.data_ptr(), G, Lmax, H, 0.125, lt.data_ptr(), None),
          "tce_mha_small64_lens_f32")
    for z, n in enumerate(lens):
        pz = planes[:, z * Lmax:z * Lmax + n].contiguous()
        ref = _alloc(n, E)
        if splits == 1:
            check(lib().tce_mha_small64_f32(pz.data_ptr(), ref.data_ptr(), n, H, 0.125, None), "tce_mha_small64_f32")
        else:
            check(lib().tce_mha_small64_splits_f32(pz.data_ptr(), splits, bp, ref.data_ptr(), n, H, 0.125, None),
                  "tce_mha_small64_splits_f32")
        torch.cuda.synchronize()
        assert torch.equal(out[z * Lmax:z * Lmax + n], ref), (splits, z)
    assert bool(torch.isfinite(out).all())  # pad rows are computed too (over the caption's keys)


# ------------------------------------------------------------------------------------------------------------- RoBERTa
@pytest.mark.parametrize("layers,lens", [(2, (9, 4, 17)), (2, (50, 20, 45))])  # 51 / 150 rows: weight-stream / tiled path
def test_text_plan_with_lengths_matches_huggingface_attention_mask(layers, lens):
    import transformers
    from tce_rvos_amd.text_encoder import TextPlan
    torch.manual_seed(layers)
    hf = transformers.RobertaModel(transformers.RobertaConfig(
        vocab_size=50265, max_position_embeddings=514, type_vocab_size=1, pad_token_id=PAD, num_hidden_layers=layers)).cuda().eval()
    ids = _padded_ids(lens, 11).cuda()
    att = (ids != PAD).long()
    G, Lmax = ids.shape
    with torch.no_grad():
        enc = hf(input_ids=ids, attention_mask=att)
        hid, pooled = TextPlan(hf).forward(ids, _alloc, lens=torch.tensor(lens, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    d1 = (hid.view(G, Lmax, -1) - enc.last_hidden_state).abs().max().item()
    d2 = (pooled - enc.pooler_output).abs().max().item()
    print("ragged text encoder max abs diff: hidden", d1, "pooled", d2)
    assert d1 < 2e-4 and d2 < 1e-4


# ------------------------------------------------------------------------------------------------------------- model
def _check_against_solo(solo, runs, G):
    for g in range(G):
        for k in solo[g]:
            ref, got = solo[g][k], runs[0][g][k]
            assert got.shape == ref.shape, (g, k, got.shape, ref.shape)
            tol = 2e-5 * float(ref.abs().max()) + 1e-6
            err = float((got - ref).abs().max())
            assert err <= tol, (g, k, err, tol)
            for r in runs[1:]:
                assert torch.equal(r[g][k], got), (g, k, "replay != eager")
        pm = solo[g]["pred_masks"]
        sure = pm.abs() > 2e-5 * float(pm.abs().max()) + 1e-6
        m_ref, m_got = (pm > 0) & sure, (runs[0][g]["pred_masks"] > 0) & sure
        inter, union = (m_ref & m_got).sum().item(), (m_ref | m_got).sum().item()
        assert union == 0 or inter / union > 0.9999, (g, inter, union)


def _ragged_case(model, clips, lens, H, W, seed=70):
    ids = _padded_ids(lens, seed).cuda()
    tgt = [{"size": torch.tensor([H, W])}]
    solo = [model([clips[g]], ids[g:g + 1, :n], tgt) for g, n in enumerate(lens)]
    solo = [{k: v.clone() for k, v in o.items() if k in GROUP_KEYS} for o in solo]
    runs = []
    for _ in range(3):  # eager, capture, replay
        outs = model.forward_group(clips, ids, tgt, ragged=True)
        torch.cuda.synchronize()
        runs.append([{k: o[k].clone() for k in GROUP_KEYS if k in o} for o in outs])
    assert len(runs[0]) == len(lens)
    _check_against_solo(solo, runs, len(lens))


@pytest.mark.parametrize("backbone,T,H,W,lens", [("swin_t_p4w7", 3, 96, 132, (9, 4, 7)),          # small
                                                 ("swin_t_p4w7", 2, 64, 96, (40, 34, 37)),        # Lmax > 32: un-folded sites
                                                 ("swin_t_p4w7", 5, 360, 640, (32, 20, 11, 7)),   # config 2 shapes
                                                 ("video_swin_t_p4w7", 4, 96, 128, (9, 5)),
                                                 ("resnet50", 1, 96, 128, (9, 3, 6))])
def test_ragged_group_matches_each_pair_alone(models, backbone, T, H, W, lens):
    model = models(backbone, 31)
    clips = [synth_frames(T, H, W, 70 + i).cuda() for i in range(len(lens))]
    _ragged_case(model, clips, lens, H, W)


def test_ragged_shared_clip_matches_each_expression_alone(models):
    model = models("swin_t_p4w7", 31)
    clip = synth_frames(3, 96, 132, 40).cuda()
    _ragged_case(model, [clip] * 4, (9, 5, 12, 6), 96, 132, seed=41)


def test_ragged_group_exact_fp32(models):
    from tce_rvos_amd import ops
    model = models("swin_t_p4w7", 31)
    try:
        ops.set_gemm_mode("f32")
        model.repack()
        clips = [synth_frames(2, 64, 96, 50 + i).cuda() for i in range(3)]
        _ragged_case(model, clips, (9, 4, 14), 64, 96, seed=51)
    finally:
        ops.set_gemm_mode("f16x3")
        model.repack()


def test_ragged_graph_follows_the_lengths_on_replay(models):
    """Capture with one length mix, replay with another of the same Lmax: the replay is the eager pass of the new mix, bit for bit,
    and the graph cache gains no entry (the lengths come from the static id buffer on every replay)."""
    model = models("swin_t_p4w7", 31)
    H, W = 96, 132
    tgt = [{"size": torch.tensor([H, W])}]
    clips = [synth_frames(3, H, W, 80 + i).cuda() for i in range(3)]
    ids_a, ids_b = _padded_ids((12, 5, 8), 81).cuda(), _padded_ids((3, 12, 10), 82).cuda()
    for _ in range(2):  # eager sighting, then the capture
        model.forward_group(clips, ids_a, tgt, ragged=True)
    torch.cuda.synchronize()
    n_graphs = len(model._graphs)
    assert any(k[0] == "group" and k[-1] == "ragged" for k in model._graphs)
    rep = [{k: o[k].clone() for k in GROUP_KEYS} for o in model.forward_group(clips, ids_b, tgt, ragged=True)]
    torch.cuda.synchronize()
    assert len(model._graphs) == n_graphs
    model.use_graph = False
    try:
        eag = [{k: o[k].clone() for k in GROUP_KEYS} for o in model.forward_group(clips, ids_b, tgt, ragged=True)]
    finally:
        model.use_graph = True
    for g in range(3):
        for k in GROUP_KEYS:
            assert torch.equal(rep[g][k], eag[g][k]), (g, k)
    solo = model([clips[0]], ids_b[:1, :3], tgt)["pred_masks"]
    assert float((rep[0]["pred_masks"] - solo).abs().max()) <= 2e-5 * float(solo.abs().max()) + 1e-6


def test_ragged_group_clips_do_not_see_each_other(models):
    model = models("swin_t_p4w7", 31)
    H, W = 96, 132
    tgt = [{"size": torch.tensor([H, W])}]
    clips = [synth_frames(3, H, W, 90 + i).cuda() for i in range(2)]
    ids = _padded_ids((7, 11), 91).cuda()
    a = {k: v.clone() for k, v in model.forward_group(clips, ids, tgt, ragged=True)[0].items() if k in GROUP_KEYS}
    ids2 = ids.clone()
    ids2[1] = _padded_ids((4,), 92, Lmax=11)[0].cuda()  # clip 1's caption: another length, same Lmax
    b = model.forward_group(clips, ids2, tgt, ragged=True)[0]
    for k in GROUP_KEYS:
        assert torch.equal(a[k], b[k]), k


def test_ragged_mode_with_equal_lengths_matches_plain_group(models):
    model = models("swin_t_p4w7", 31)
    H, W = 96, 132
    tgt = [{"size": torch.tensor([H, W])}]
    clips = [synth_frames(3, H, W, 95 + i).cuda() for i in range(3)]
    ids = _padded_ids((9, 9, 9), 96).cuda()
    plain = model.forward_group(clips, ids, tgt)
    rag = model.forward_group(clips, ids, tgt, ragged=True)
    for g in range(3):
        for k in GROUP_KEYS:
            ref = plain[g][k]
            assert float((rag[g][k] - ref).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-6, (g, k)


def test_ragged_strings_and_host_validation(models):
    model = models("swin_t_p4w7", 31)
    H, W = 96, 128
    tgt = [{"size": torch.tensor([H, W])}]
    clips = [synth_frames(3, H, W, 60 + i).cuda() for i in range(2)]
    caps = ["a dog", "a dog running on the grass"]
    outs = model.forward_group(clips, caps, tgt, ragged=True)
    for g, c in enumerate(caps):
        solo = model([clips[g]], [c], tgt)["pred_masks"]
        assert float((outs[g]["pred_masks"] - solo).abs().max()) <= 2e-5 * float(solo.abs().max()) + 1e-6
    with pytest.raises(ValueError):  # interior pad on the host
        model.forward_group(clips, torch.tensor([[0, 7, PAD, 9, 2], [0, 7, 8, 9, 2]]), tgt, ragged=True)
    with pytest.raises(ValueError):  # a caption with no token
        model.forward_group(clips, torch.tensor([[PAD, PAD, PAD], [0, 7, 2]]), tgt, ragged=True)
    with pytest.raises(ValueError):  # without the keyword: still rejected
        model.forward_group(clips, caps, tgt)


@pytest.mark.parametrize("G,T,H,W", [(3, 3, 96, 132), (4, 5, 360, 640)])
def test_ragged_launch_program_is_race_free(models, G, T, H, W):
    model = models("swin_t_p4w7", 5)
    clips = [synth_frames(T, H, W, 30 + i).cuda() for i in range(G)]
    ids = _padded_ids((32, 20, 11, 7)[:G], 31).cuda()
    rep = model.hazard_check(torch.cat(clips, 0), ids, (H, W), groups=G, ragged=True)
    print(rep)
    assert rep.launches > 200 and rep.unordered_pairs > 1000
    assert rep.clean, str(rep)


def test_run_video_expressions_mixed_lengths(models):
    from tce_rvos_amd.video import run_video, run_video_expressions
    model = models("swin_t_p4w7", 31)
    H, W, H0, W0 = 96, 128, 180, 240
    frames = synth_frames(7, H, W, 90).cuda()
    caps = ["the left zebra", "a person walking a dog", "the right zebra", "the small dog", "a car"]   # lengths 5, 7, 5, 5, 4
    calls = []
    orig = model.forward_group

    def counting(*a, **k):
        calls.append(k.get("ragged", False))
        return orig(*a, **k)
    model.forward_group = counting
    try:
        res = run_video_expressions(model, frames, caps, (H0, W0), clip_size=4, max_group=4, mixed_lengths=True)
        n_mixed = len(calls)
        run_video_expressions(model, frames, caps, (H0, W0), clip_size=4, max_group=4)
        n_bucketed = len(calls) - n_mixed
    finally:
        del model.forward_group
    assert all(calls[:n_mixed]) and not any(calls[n_mixed:])
    assert (n_mixed, n_bucketed) == (2 * 2, 3 * 2)  # 2 chunks of the 7 frames
    assert len(res) == len(caps)
    for c, r in zip(caps, res):
        ref = run_video(model, frames, c, (H0, W0), clip_size=4)
        assert torch.equal(r["best_query"], ref["best_query"]), c
        assert r["masks"].shape == ref["masks"].shape == (7, H0, W0)
        assert (r["masks"] != ref["masks"]).float().mean().item() < 1e-4, c
        assert float((r["pred_logits"] - ref["pred_logits"]).abs().max()) < 1e-4
