"""Ragged clip groups (captions of different token length in one forward_group) -- the host side: padding / validation rules,
the expression grouping plan of run_video_expressions, the hazard access models of the new entry points and the 1-D position
table restated in torch against the reference's own PositionEmbeddingSine1D (tests/golden/text_pos_ragged.npz)."""
import math
import os

import numpy as np
import pytest
import torch

from tce_rvos_amd import _lib, hazard
from tce_rvos_amd.hazard import dense, union
from tce_rvos_amd.model import caption_lengths, pad_captions
from tce_rvos_amd.video import plan_expression_groups

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAD = 1


def test_pad_captions_right_pads_to_the_longest():
    rows = [torch.tensor([[0, 11, 12, 2]]), torch.tensor([[0, 2]]), torch.tensor([[0, 5, 6, 7, 8, 2]])]
    ids, lens = pad_captions(rows, PAD)
    assert lens == [4, 2, 6]
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (3, 6)
    assert ids[0].tolist() == [0, 11, 12, 2, PAD, PAD]
    assert ids[1].tolist() == [0, 2, PAD, PAD, PAD, PAD]
    assert ids[2].tolist() == [0, 5, 6, 7, 8, 2]
    assert caption_lengths(ids, PAD) == lens


def test_caption_lengths_rules_and_rejections():
    ids = torch.tensor([[0, 7, 2, PAD], [0, 7, 8, 2]])
    assert caption_lengths(ids, PAD) == [3, 4]
    with pytest.raises(ValueError):  # interior pad
        caption_lengths(torch.tensor([[0, PAD, 9, 2]]), PAD)
    with pytest.raises(ValueError):  # a caption with no token
        caption_lengths(torch.tensor([[PAD, PAD, PAD]]), PAD)
    with pytest.raises(ValueError):
        caption_lengths(torch.tensor([0, 2]), PAD)  # not [G, Lmax]
    with pytest.raises(ValueError):  # a row that carries the pad id itself
        pad_captions([torch.tensor([[0, PAD, 2]]), torch.tensor([[0, 2]])], PAD)
    with pytest.raises(ValueError):  # an empty row
        pad_captions([torch.zeros(1, 0, dtype=torch.long), torch.tensor([[0, 2]])], PAD)


def test_expression_grouping_plan():
    lens = [5, 7, 5, 5, 4]  # the captions of test_run_video_expressions_matches_run_video
    assert plan_expression_groups(lens, 2) == [[0, 2], [3], [1], [4]]
    assert plan_expression_groups(lens, 4) == [[0, 2, 3], [1], [4]]
    assert plan_expression_groups(lens, 4, mixed_lengths=True) == [[0, 1, 2, 3], [4]]
    assert plan_expression_groups(lens, 2, mixed_lengths=True) == [[0, 1], [2, 3], [4]]
    assert plan_expression_groups(lens, 0, mixed_lengths=True) == [[0], [1], [2], [3], [4]]
    assert plan_expression_groups([], 4, mixed_lengths=True) == []
    for mg in (1, 3, 8):
        for mixed in (False, True):
            plan = plan_expression_groups(lens, mg, mixed)
            assert sorted(i for g in plan for i in g) == list(range(len(lens)))
            assert all(1 <= len(g) <= mg for g in plan)


def _sz(iv):
    return int((iv[:, 1] - iv[:, 0]).sum())


def test_hazard_models_of_the_ragged_entry_points():
    for name in ("tce_caption_lens_f32", "tce_mha_small64_lens_f32", "tce_xattn_pack_lens_f32", "tce_xattn_prepare_lens_f32"):
        assert name in _lib.SIGNATURES and name in hazard.MODELS, name
    G, Lmax, D = 3, 17, 256
    rd, wr = hazard.MODELS["tce_caption_lens_f32"]((0x1000, G, Lmax, PAD, D, 0x10000, 0x20000, 0x30000, 0))
    assert _sz(union(*rd)) == G * Lmax * 8
    assert [_sz(w) for w in wr] == [G * 4, G * Lmax, G * Lmax * D * 4]
    # planes, splits, bias, out, nseq, L, nheads, scale, lens
    rd, wr = hazard.MODELS["tce_mha_small64_lens_f32"]((0x100000, 3, 0x900000, 0xA00000, G, Lmax, 12, 0.125, 0xB00000, 0))
    assert [_sz(r) for r in rd] == [3 * G * Lmax * 3 * 768 * 4, 3 * 768 * 4, G * 4]
    assert _sz(union(*wr)) == G * Lmax * 768 * 4
    rd, wr = hazard.MODELS["tce_mha_small64_lens_f32"]((0x100000, 1, None, 0xA00000, G, Lmax, 12, 0.125, 0xB00000, 0))
    assert [_sz(r) for r in rd] == [G * Lmax * 3 * 768 * 4, 0, G * 4]
    # k, v, wqT, wo, packed, L, group, batch, lens: the lengths are read, the streams written
    L, group = 20, 32
    rd, wr = hazard.MODELS["tce_xattn_pack_lens_f32"]((0x100000, 0x200000, 0x300000, 0x400000, 0x800000, L, group, G, 0x700000, 0))
    plain_rd, plain_wr = hazard.MODELS["tce_xattn_pack_f32"]((0x100000, 0x200000, 0x300000, 0x400000, 0x800000, L, group, G, 0))
    assert len(rd) == 5 and all(np.array_equal(a, b) for a, b in zip(rd[:4], plain_rd))
    assert np.array_equal(rd[4], dense(0x700000, G * 4))
    assert np.array_equal(union(*wr), union(*plain_wr))
    # k, v, wqT, wo, W1, b1, W2, L, group, batch, lens
    rd, wr = hazard.MODELS["tce_xattn_prepare_lens_f32"]((0x100000, 0x200000, 0x300000, 0x400000, 0x800000, 0x900000, 0xA00000,
                                                          L, 8, G, 0x700000, 0))
    assert np.array_equal(rd[4], dense(0x700000, G * 4))
    assert [_sz(w) for w in wr] == [G * 64 * 256 * 4, G * 64 * 4, G * 64 * 256 * 4]


def text_pos_ragged(lens, Lmax, D=256):
    """The tce_caption_lens_f32 position table restated in torch: x = min(j + 1, n) / (n + 1e-6) * 2 pi (the masked cumulative
    sum of PositionEmbeddingSine1D normalised by its last entry), sin / cos interleaved."""
    out = []
    for n in lens:
        x = torch.clamp(torch.arange(1, Lmax + 1, dtype=torch.float32), max=float(n))
        x = x / (torch.tensor(float(n)) + 1e-6) * (2 * math.pi)
        dim_t = torch.arange(D, dtype=torch.float32)
        dim_t = 10000.0 ** (2 * torch.div(dim_t, 2, rounding_mode="trunc") / D)
        px = x[:, None] / dim_t
        out.append(torch.stack((px[:, 0::2].sin(), px[:, 1::2].cos()), dim=2).flatten(1))
    return torch.stack(out, 0)


def test_position_table_matches_the_reference_fixture():
    fx = np.load(os.path.join(GOLDEN, "text_pos_ragged.npz"))
    lens, mask, pos = fx["lens"].tolist(), fx["mask"], fx["pos"]
    Lmax = mask.shape[1]
    assert len(set(lens)) == 3 and max(lens) == Lmax
    assert np.array_equal(mask, np.arange(Lmax)[None, :] >= np.array(lens)[:, None])
    got = text_pos_ragged(lens, Lmax).numpy()
    assert got.shape == pos.shape
    assert float(np.abs(got - pos).max()) < 2e-6
