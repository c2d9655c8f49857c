"""GPU: captions of 129..512 tokens.  The key-tiled form of the text self-attention kernel (csrc/text.hip, mha_tiled_kernel, tiles of
TILE = 64 keys, behind the four tce_mha_small64_* entry points) against the fp64 references and the derived bounds of tests/_text.py
(unchanged: the bound grows with the number of keys as derived there, nothing is widened here); ragged launches against solo
launches bit for bit; RoBERTa on the HIP kernels against HuggingFace at 130 and 512 tokens; the whole forward on a 160-token caption
against the reference's own output (tests/golden/e2e_swin_t_long_caption.npz), eager and as a graph replay; a ragged group of a 6-
and a 160-token caption, the expressions driver over it, the other drivers and the hazard checker.

Lengths.  Up to 128 tokens the launchers take the whole-sentence kernel, so tile edges below 129 (TILE +- 1, 2 TILE - 1) belong to
tests/test_text_kernels_gpu.py, which runs them; here: 129 = 2 TILE + 1 (one key in the third tile), 3 TILE - 1 / 3 TILE / 3 TILE + 1,
4 TILE - 1 / + 1, 511, 512, and 130 with two heads (a last query block of two rows)."""
import pytest
import torch

import _text as K
from _util import synth_frames

pytestmark = pytest.mark.gpu

TILE = 64
PAD = 1


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tce_rvos_amd._lib import lib as load
    return load()


def run_mha(lib, c, entry=None, planes=None, L=None, lens=None):
    """This file's runner (the one of tests/test_text_kernels_gpu.py stops at 128 tokens): the case through its entry point (or through
    `entry`, on `planes` [splits, nseq' * L, 3E]).  Returns the whole guarded buffer [nseq' * L + GUARD, E] on the host: every element
    starts as NaN, the GUARD rows after the output must still be NaN afterwards."""
    from tce_rvos_amd._lib import check
    entry = entry or c["entry"]
    planes = (c["planes"] if planes is None else planes).cuda().contiguous()
    L = L or c["L"]
    H, splits, scale = c["nheads"], planes.shape[0], c["scale"]
    nseq = planes.shape[1] // L
    assert planes.shape[1] == nseq * L and planes.shape[2] == 3 * H * K.HD and 1 <= L <= 512 and 1 <= splits <= 64 and 1 <= nseq <= 64
    bias = None if c["bias"] is None else c["bias"].cuda()
    bp = None if bias is None else bias.data_ptr()
    out = torch.full((nseq * L + K.GUARD, H * K.HD), float("nan"), device="cuda")
    if entry == "plain":
        assert splits == 1 and bias is None and nseq == 1
        st = lib.tce_mha_small64_f32(planes.data_ptr(), out.data_ptr(), L, H, scale, None)
    elif entry == "splits":
        assert nseq == 1
        st = lib.tce_mha_small64_splits_f32(planes.data_ptr(), splits, bp, out.data_ptr(), L, H, scale, None)
    elif entry == "seqs":
        st = lib.tce_mha_small64_seqs_f32(planes.data_ptr(), splits, bp, out.data_ptr(), nseq, L, H, scale, None)
    else:
        assert entry == "lens"
        lt = torch.tensor(c["lens"] if lens is None else lens, dtype=torch.int32).cuda()
        assert lt.numel() == nseq
        st = lib.tce_mha_small64_lens_f32(planes.data_ptr(), splits, bp, out.data_ptr(), nseq, L, H, scale, lt.data_ptr(), None)
    check(st, "tce_mha_small64 " + entry)
    torch.cuda.synchronize()
    return out.cpu()


# (family, heads, L, keywords of _text.mha_case)
MHA_CASES = [
    ("dom_first", 1, 2 * TILE + 1, {}),                 # 129: the dominant key in the first tile, its maximum carried over two more
    ("dom_last", 12, 2 * TILE + 1, {}),                 # the dominant key alone in the last tile; every head of RoBERTa-base
    ("wide", 2, 130, {}),                               # two heads, a last query block of two rows
    ("ascending", 1, 3 * TILE - 1, {}),                 # the maximum moves at every key, across every tile edge
    ("descending", 1, 3 * TILE, {}),
    ("dom_last", 1, 3 * TILE + 1, {}),
    ("ascending", 1, 4 * TILE - 1, {}),
    ("dom_first", 1, 4 * TILE + 1, {}),
    ("descending", 1, 511, {}),
    ("ascending", 1, 512, {}),
    ("dom_last", 1, 512, {}),
    ("uniform", 2, 3 * TILE + 1, dict(nseq=2)),
    ("dom_first", 1, 2 * TILE + 1, dict(splits=3, bias=True)),
    ("descending", 2, 4 * TILE + 1, dict(nseq=2, splits=3, bias=True, scale=0.1)),
    # lens: K / V rows past each length are NaN; 0 and Lmax + 5 are the clamp
    ("dom_lkm1", 1, 300, dict(nseq=2, lens=(5, 300))),                                   # a pair straddling tile edges
    ("wide", 2, 200, dict(nseq=4, splits=3, bias=True, lens=(1, 128, 129, 200))),
    ("ascending", 1, 512, dict(nseq=3, lens=(TILE, TILE + 1, 512))),
    ("dom_first", 1, 130, dict(nseq=2, lens=(0, 135))),
]
MHA_IDS = [f"{f}-H{h}-L{L}" + "".join(f"-{k}{v}" for k, v in kw.items()).replace(" ", "") for f, h, L, kw in MHA_CASES]


@pytest.mark.parametrize("family,heads,L,kw", MHA_CASES, ids=MHA_IDS)
def test_tiled_mha_inside_the_bound(lib, family, heads, L, kw):
    c = K.mha_case(family, heads, L, seed=L, **kw)
    ref, B, _ = K.mha_ref_and_bound(c)
    out = run_mha(lib, c)
    n = ref.shape[0]
    r = K.ratio(c, out, (ref, B))
    print(f"{c['entry']} | {c['name']} | worst err / B = {r:.3f}")
    assert bool(torch.isnan(out[n:]).all()), "sentinel rows written"
    assert bool(torch.isfinite(out[:n]).all()), f"{int((~torch.isfinite(out[:n])).sum())} elements not finite"
    assert r <= 1.0, f"worst err / B = {r:.3g}"


def test_families_that_stress_the_carried_maximum_all_ran():
    assert {"dom_first", "dom_last", "ascending", "descending"} <= {f for f, _, _, _ in MHA_CASES} <= set(K.MHA_FAMILIES)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("lens", [(5, 200), (128, 129), (129, 130, 65)])
def test_ragged_sequence_equals_its_solo_launch_bit_for_bit(lib, lens, splits):
    """Sequence z of a lens launch at Lmax > 128 (the tiled kernel) against the plain launch at L = lens[z] -- the whole-sentence kernel
    for 5, 65 and 128 tokens, the tiled one above: both walk their keys through one inlined body (mha_fold_keys), key by key."""
    Lmax = max(lens)
    c = K.mha_case("wide", 2, Lmax, nseq=len(lens), splits=splits, bias=splits > 1, lens=lens, seed=7)
    planes = c["planes"].nan_to_num(nan=0.5)  # the solo launches see the rows only up to lens[z]; NaN past them is the other test's
    out = run_mha(lib, c, planes=planes)
    for z, n in enumerate(lens):
        pz = planes[:, z * Lmax:z * Lmax + n].contiguous()
        solo = run_mha(lib, c, entry="plain" if splits == 1 else "splits", planes=pz, L=n)
        assert torch.equal(out[z * Lmax:z * Lmax + n], solo[:n]), (lens, splits, z)
    assert bool(torch.isfinite(out[:len(lens) * Lmax]).all())  # pad rows are computed too, over the caption's keys


# ---------------------------------------------------------------------------------------------------------------------
# RoBERTa on the HIP kernels against HuggingFace
# ---------------------------------------------------------------------------------------------------------------------
def _alloc(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="cuda")


@pytest.mark.parametrize("layers,lens", [(2, (130,)), (1, (512,)), (2, (130, 40)), (1, (129, 512))])
def test_text_plan_matches_huggingface(layers, lens):
    """As test_text_plan_with_lengths_matches_huggingface_attention_mask (tests/test_ragged_captions_gpu.py), with its bound: one
    caption without lengths, two right-padded ones with."""
    import transformers
    from test_ragged_captions_gpu import _padded_ids
    from tce_rvos_amd.text_encoder import TextPlan
    torch.manual_seed(layers)
    hf = transformers.RobertaModel(transformers.RobertaConfig(
        vocab_size=50265, max_position_embeddings=514, type_vocab_size=1, pad_token_id=PAD, num_hidden_layers=layers)).cuda().eval()
    ids = _padded_ids(lens, 11).cuda()
    G, Lmax = ids.shape
    lt = torch.tensor(lens, dtype=torch.int32).cuda() if G > 1 else None
    with torch.no_grad():
        enc = hf(input_ids=ids, attention_mask=(ids != PAD).long())
        hid, pooled = TextPlan(hf).forward(ids, _alloc, lens=lt)
    torch.cuda.synchronize()
    d1 = (hid.view(G, Lmax, -1) - enc.last_hidden_state).abs().max().item()
    d2 = (pooled.view(G, -1) - enc.pooler_output).abs().max().item()
    print("text encoder max abs diff: hidden", d1, "pooled", d2)
    assert d1 < 2e-4 and d2 < 1e-4


def test_text_plan_refuses_a_caption_beyond_the_position_table():
    import transformers
    from tce_rvos_amd.text_encoder import TextPlan
    hf = transformers.RobertaModel(transformers.RobertaConfig(
        vocab_size=100, max_position_embeddings=514, type_vocab_size=1, pad_token_id=PAD, num_hidden_layers=1)).cuda().eval()
    with pytest.raises(ValueError, match=r"513 tokens.*at most 512"):
        TextPlan(hf).forward(torch.full((1, 513), 5, dtype=torch.int64, device="cuda"), _alloc)


# ---------------------------------------------------------------------------------------------------------------------
# through the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    from test_e2e_gpu import _args
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


def _seeded_roberta_state(seed):
    """tests/golden/make_golden_long_caption.py, seeded_roberta_state: the one-layer RoBERTa the fixture was made with (its weights
    are not synthetic and far too large to store: HuggingFace's initialisation under a seed of its own, on the host)."""
    import transformers
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        cfg = transformers.RobertaConfig(vocab_size=50265, max_position_embeddings=514, type_vocab_size=1, pad_token_id=1,
                                         num_hidden_layers=1)
        return transformers.RobertaModel(cfg).state_dict()


def test_long_caption_forward_matches_reference_eager_and_replayed(models):
    """The reference's own forward on a 160-token caption (make_golden_long_caption.py), held with the helper and the bounds of
    test_swin_t_small_matches_reference: from the reference's text features as that test runs, and from the token ids through
    RoBERTa on the HIP kernels; then the same forward captured and replayed, bit for bit the eager one."""
    from test_e2e_gpu import _compare, _run
    fx, out, model = _run(models, "e2e_swin_t_long_caption.npz", "swin_t_p4w7")
    _compare(out, fx, 5e-3)
    T, H, W = (int(v) for v in fx["thw"])
    ids = torch.from_numpy(fx["ids"])
    assert tuple(ids.shape) == (1, 160) and int(ids[0, 0]) == 0 and int(ids[0, -1]) == 2
    frames = synth_frames(T, H, W, int(fx["frames_seed"])).cuda()
    tgt = [{"size": torch.tensor([H, W])}]
    model.text_encoder.load_state_dict(_seeded_roberta_state(int(fx["text_seed"])))  # the fixture's text encoder, from its seed
    model._text = None  # the text plan keeps packed copies of the old weights
    hid, pooled = model.forward_text_encoder(ids.cuda(), "cuda")
    torch.cuda.synchronize()
    d1 = (hid.reshape(160, -1).cpu() - torch.from_numpy(fx["text_hidden"])[0]).abs().max().item()
    d2 = (pooled.reshape(-1).cpu() - torch.from_numpy(fx["text_pooled"])[0]).abs().max().item()
    print("text features vs reference: hidden", d1, "pooled", d2)
    assert d1 < 2e-4 and d2 < 1e-4  # the bound of test_text_encoder_hip_matches_huggingface
    n_graphs = len(model._graphs)
    outs = []
    for _ in range(4):  # eager sighting, capture, replays
        o = model([frames], ids.cuda(), tgt)
        torch.cuda.synchronize()
        outs.append({k: o[k].clone() for k in ("pred_logits", "pred_boxes", "pred_masks", "memory", "reference_points")})
    _compare(outs[0], fx, 5e-3)
    assert len(model._graphs) == n_graphs + 1 and not model._nograph  # captured: the text branch's arena took 160 tokens
    for o in outs[1:]:
        for k, v in o.items():
            assert torch.equal(v, outs[0][k]), k


def test_ragged_group_of_a_short_and_a_long_caption(models):
    """forward_group(..., ragged=True) of a 6- and a 160-token caption: each result is its own forward on the un-padded caption,
    within the bound of test_ragged_group_matches_each_pair_alone (its helper), eager, captured and replayed."""
    from test_ragged_captions_gpu import _ragged_case
    model = models("swin_t_p4w7", 31)
    clips = [synth_frames(2, 64, 96, 70 + i).cuda() for i in range(2)]
    _ragged_case(model, clips, (6, 160), 64, 96)


def test_run_video_expressions_mixed_lengths_with_a_long_caption(models):
    """The expressions driver on a 4-frame video with a 6- and a 160-token caption equals its planned forwards called by hand: one
    ragged group of the two captions per chunk of two frames."""
    from test_ragged_captions_gpu import _padded_ids
    from tce_rvos_amd import ops
    from tce_rvos_amd.video import plan_expression_groups, run_video_expressions
    model = models("swin_t_p4w7", 31)
    H, W, H0, W0 = 64, 96, 90, 120
    frames = synth_frames(4, H, W, 90).cuda()
    caps = [_padded_ids((6,), 1), _padded_ids((160,), 2)]
    assert plan_expression_groups([6, 160], 4, True) == [[0, 1]]
    res = run_video_expressions(model, frames, caps, (H0, W0), clip_size=2, max_group=4, mixed_lengths=True)
    torch.cuda.synchronize()
    tok = _padded_ids((6, 160), 0)
    tok[0, :6], tok[1] = caps[0][0], caps[1][0]
    tgt = [{"size": torch.tensor([H, W])}]
    want = [dict(masks=[], best_query=[], pred_logits=[]) for _ in caps]
    for lo in (0, 2):
        outs = model.forward_group([frames[lo:lo + 2]] * 2, tok.cuda(), tgt, ragged=True)
        for w, o in zip(want, outs):
            m, b = ops.select_masks(o["pred_logits"][0], o["pred_masks"][0], (H0, W0), 0.5)
            w["masks"].append(m)
            w["best_query"].append(b)
            w["pred_logits"].append(o["pred_logits"][0][torch.arange(2, device="cuda"), b.long().expand(2)])
    torch.cuda.synchronize()
    assert len(res) == 2
    for r, w in zip(res, want):
        assert r["masks"].shape == (4, H0, W0)
        for k, v in w.items():
            assert torch.equal(r[k], torch.cat(v, 0)), k
    # bucketed by length (the default): each caption alone, through forward
    res2 = run_video_expressions(model, frames, caps, (H0, W0), clip_size=2, max_group=4)
    for a, b in zip(res, res2):
        assert torch.equal(a["best_query"], b["best_query"])
        assert (a["masks"] != b["masks"]).float().mean().item() < 1e-4


def test_other_drivers_and_the_text_cache_take_a_long_caption(models):
    from test_ragged_captions_gpu import _padded_ids
    from tce_rvos_amd.video import run_video, run_video_windows
    model = models("swin_t_p4w7", 31)
    H, W, H0, W0 = 64, 96, 90, 120
    frames = synth_frames(4, H, W, 91).cuda()
    ids = _padded_ids((160,), 3)  # host ids: the text cache's key
    ref = run_video(model, frames, ids, (H0, W0), clip_size=2)
    assert ref["masks"].shape == (4, H0, W0) and bool(torch.isfinite(ref["pred_logits"]).all())
    win = run_video_windows(model, frames, ids, (H0, W0), num_frames=2, f_extra=0)
    assert torch.equal(win["best_query"], ref["best_query"])  # windows without context frames are run_video's chunks
    assert (win["masks"] != ref["masks"]).float().mean().item() < 1e-4
    model.text_cache_size = 2
    try:
        cached = run_video(model, frames, ids, (H0, W0), clip_size=2)
        assert len(model._text_cache) == 1
    finally:
        model.text_cache_size = 0
        model._text_cache.clear()
    assert torch.equal(cached["best_query"], ref["best_query"])
    assert float((cached["pred_logits"] - ref["pred_logits"]).abs().max()) < 1e-4


def test_indexed_group_with_a_long_caption(models):
    """forward_indexed of two windows of a 3-frame pool under a 6- and a 160-token caption (ragged): each slot is its own forward."""
    from test_ragged_captions_gpu import GROUP_KEYS, _padded_ids
    model = models("swin_t_p4w7", 31)
    H, W = 64, 96
    pool = synth_frames(3, H, W, 92).cuda()
    index = [(0, 1), (1, 2)]
    ids = _padded_ids((6, 160), 4).cuda()
    tgt = [{"size": torch.tensor([H, W])}]
    outs = model.forward_indexed(pool, index, ids, tgt, ragged=True)
    for g, n in enumerate((6, 160)):
        solo = model([pool[list(index[g])]], ids[g:g + 1, :n], tgt)
        for k in GROUP_KEYS:
            ref = solo[k]
            assert float((outs[g][k] - ref).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-6, (g, k)


def test_launch_program_is_race_free_at_160_tokens(models):
    from test_ragged_captions_gpu import _padded_ids
    model = models("swin_t_p4w7", 5)
    T, H, W = 2, 64, 96
    rep = model.hazard_check(synth_frames(T, H, W, 30).cuda(), _padded_ids((160,), 5).cuda(), (H, W))
    print(rep)
    assert rep.launches > 100
    assert rep.clean, str(rep)
