"""CPU: captions of more than 128 tokens (up to RoBERTa's 512) -- what can be checked without a GPU: the four tce_mha_small64_*
entry points refuse L = 513 before any launch with a message that names 512, the boundaries refuse a caption beyond the text
encoder's limit as an argument error (before the device of the inputs matters), and the access models of the four entries give
the extents of a 512-token launch."""
import argparse

import pytest
import torch

from tce_rvos_amd import _lib, hazard
from tce_rvos_amd.hazard import union

P = 0x100000  # 16-byte aligned stand-ins for device pointers: nothing is launched, nothing dereferenced


def _sz(iv):
    return int((iv[:, 1] - iv[:, 0]).sum())


@pytest.mark.parametrize("name,args", [
    # qkv, out, L, nheads, scale
    ("tce_mha_small64_f32", lambda L: (P, 2 * P, L, 12, 0.125)),
    # planes, splits, bias, out, L, nheads, scale
    ("tce_mha_small64_splits_f32", lambda L: (P, 3, 3 * P, 2 * P, L, 12, 0.125)),
    # planes, splits, bias, out, nseq, L, nheads, scale
    ("tce_mha_small64_seqs_f32", lambda L: (P, 3, 3 * P, 2 * P, 2, L, 12, 0.125)),
    # planes, splits, bias, out, nseq, L, nheads, scale, lens
    ("tce_mha_small64_lens_f32", lambda L: (P, 3, 3 * P, 2 * P, 2, L, 12, 0.125, 4 * P)),
])
def test_entry_points_refuse_513_tokens_and_name_512(name, args):
    lib = _lib.lib_raw()
    for L in (513, 0):
        assert getattr(lib, name)(*args(L), None) != 0
        msg = lib.tce_last_error().decode()
        assert name in msg and "512" in msg and str(L) in msg, msg
    with pytest.raises(_lib.TceError, match="512"):
        _lib.check(getattr(lib, name)(*args(513), None), name)


@pytest.fixture(scope="module")
def model():
    from tce_rvos_amd import build_model
    args = argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)
    m, _, _ = build_model(args)
    return m.eval()


def _ids(G, L):
    ids = torch.randint(3, 50000, (G, L), generator=torch.Generator().manual_seed(L))
    ids[:, 0], ids[:, -1] = 0, 2
    return ids


def test_caption_limit_is_the_position_table_and_the_kernel():
    from tce_rvos_amd.text_encoder import max_caption_tokens
    assert max_caption_tokens(514, 1) == 512      # RoBERTa: positions pad + 1 .. pad + L inside 514 rows
    assert max_caption_tokens(130, 1) == 128      # a shorter table rules
    assert max_caption_tokens(1026, 1) == 512     # a longer one does not lift the attention kernels' limit


def test_forward_refuses_513_tokens_as_an_argument_error(model):
    H, W = 32, 48
    clip, tgt = torch.zeros(2, 3, H, W), [{"size": torch.tensor([H, W])}]
    with pytest.raises(ValueError, match=r"513 tokens.*at most 512"):
        model.forward([clip], _ids(1, 513), tgt)
    with pytest.raises(RuntimeError, match="GPU"):  # 512 tokens are fine: only now does the device matter
        model.forward([clip], _ids(1, 512), tgt)


@pytest.mark.parametrize("ragged", [False, True])
def test_forward_group_refuses_513_tokens_as_an_argument_error(model, ragged):
    H, W = 32, 48
    clips, tgt = [torch.zeros(2, 3, H, W)] * 2, [{"size": torch.tensor([H, W])}]
    with pytest.raises(ValueError, match=r"513 tokens.*at most 512"):
        model.forward_group(clips, _ids(2, 513), tgt, ragged=ragged)
    with pytest.raises(ValueError, match="CUDA tensors"):  # the group's own device check comes after the captions
        model.forward_group(clips, _ids(2, 512), tgt, ragged=ragged)
    with pytest.raises(ValueError, match=r"513 tokens.*at most 512"):  # G = 1 goes to forward
        model.forward_group(clips[:1], _ids(1, 513), tgt, ragged=ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_forward_indexed_refuses_513_tokens_as_an_argument_error(model, ragged):
    H, W = 32, 48
    pool, tgt, index = torch.zeros(4, 3, H, W), [{"size": torch.tensor([H, W])}], [(0, 1), (2, 3)]
    with pytest.raises(ValueError, match=r"513 tokens.*at most 512"):
        model.forward_indexed(pool, index, _ids(2, 513), tgt, ragged=ragged)
    with pytest.raises(RuntimeError, match="GPU"):
        model.forward_indexed(pool, index, _ids(2, 512), tgt, ragged=ragged)


def test_text_arena_grows_with_long_captions_only(model):
    assert model._text_arena_extra(None) == 0 and model._text_arena_extra((1, 32)) == 0 and model._text_arena_extra((64, 128)) == 0
    # one 512-token caption: RoBERTa's rows alone (x, qkv, attention output, hidden, one workspace) are 512 * 4 * 11 * 768 bytes
    assert model._text_arena_extra((1, 512)) > 512 * 4 * 11 * 768
    assert model._text_arena_extra((2, 512)) > 2 * 512 * 4 * 11 * 768


def test_hazard_models_at_512_tokens():
    """The extents a 512-token launch touches, restated by hand: E = 12 * 64 floats per row of the output, 3E per row of a plane."""
    L, H, E, F = 512, 12, 768, 4
    # qkv, out, L, nheads, scale
    rd, wr = hazard.MODELS["tce_mha_small64_f32"]((P, 16 * P, L, H, 0.125, 0))
    assert [_sz(r) for r in rd] == [L * 3 * E * F] and _sz(union(*wr)) == L * E * F
    assert int(rd[0][0, 0]) == P and int(wr[0][0, 0]) == 16 * P
    # planes, splits, bias, out, L, nheads
    rd, wr = hazard.MODELS["tce_mha_small64_splits_f32"]((P, 3, 15 * P, 16 * P, L, H, 0.125, 0))
    assert [_sz(r) for r in rd] == [3 * L * 3 * E * F, 3 * E * F] and _sz(union(*wr)) == L * E * F
    # planes, splits, bias, out, nseq, L, nheads
    rd, wr = hazard.MODELS["tce_mha_small64_seqs_f32"]((P, 1, None, 16 * P, 2, L, H, 0.125, 0))
    assert [_sz(r) for r in rd] == [2 * L * 3 * E * F, 0] and _sz(union(*wr)) == 2 * L * E * F
    # planes, splits, bias, out, nseq, L, nheads, scale, lens: every row is written, pad rows included
    rd, wr = hazard.MODELS["tce_mha_small64_lens_f32"]((P, 3, 15 * P, 32 * P, 2, L, H, 0.125, 31 * P, 0))
    assert [_sz(r) for r in rd] == [3 * 2 * L * 3 * E * F, 3 * E * F, 2 * 4] and _sz(union(*wr)) == 2 * L * E * F
