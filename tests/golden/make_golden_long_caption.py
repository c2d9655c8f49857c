"""Generates tests/golden/e2e_swin_t_long_caption.npz by running the REFERENCE's own forward on a 160-token caption (CPU, build
machine only).

Run from the repository root:  python tests/golden/make_golden_long_caption.py
Needs the reference tree (ref_harness.REF_ROOT) -- never runs on the GPU box.  The file it writes is data:

  e2e_swin_t_long_caption.npz  full ReferFormer.forward of the reference at the shape and model arguments of e2e_swin_t_small.npz
                               (make_golden.gen_e2e: real Swin-T, T=3, 72x100, one RoBERTa layer, synthetic weights of salt 0,
                               frames of seed 1), but the tokenizer stand-in returns ONE caption of 160 token ids -- more than the
                               128 tokens the text self-attention kernel held in LDS, fewer than RoBERTa's 512 positions -- and
                               the text encoder's weights (which the synthetic weights leave alone, and which are far too large
                               to store) are those of seeded_roberta_state(): a test rebuilds them from the seed and runs the
                               forward from the token ids, RoBERTa included:
                                 ids [1, 160] int64 (seeded, 3..50000, <s> = 0 first, </s> = 2 last; no pad id),
                                 text_hidden [1, 160, 768], text_pooled [1, 768] (the reference's RoBERTa outputs),
                                 out_pred_logits / out_pred_boxes / out_pred_masks / out_reference_points, out_memory_abs_sum,
                                 text_seed (of seeded_roberta_state), thw, frames_seed, weights_salt, cfg_backbone as in
                                 e2e_swin_t_small.npz
                               (no aux outputs and no stage maps: the file stays smaller than e2e_swin_t_small.npz).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

L = 160
IDS_SEED = 160
TEXT_SEED = 1160
BACKBONE, T, H, W, SEED = "swin_t_p4w7", 3, 72, 100, 0  # make_golden.py: e2e_swin_t_small.npz


def long_caption_ids():
    g = torch.Generator().manual_seed(IDS_SEED)
    ids = torch.randint(3, 50001, (1, L), generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    return ids


def seeded_roberta_state(seed=TEXT_SEED):
    """State dict of a one-layer RobertaModel initialised by HuggingFace under a seed of its own (the global generator is restored)."""
    import transformers
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        cfg = transformers.RobertaConfig(vocab_size=50265, max_position_embeddings=514, type_vocab_size=1, pad_token_id=1,
                                         num_hidden_layers=1)
        return transformers.RobertaModel(cfg).state_dict()


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tce_rvos_amd.weights import load_synth_weights
    ids = long_caption_ids()
    model = rh.build_reference_model(rh.reference_args(BACKBONE), seed=0, roberta_layers=1, token_ids=ids)
    load_synth_weights(model, salt=SEED)
    model.text_encoder.load_state_dict(seeded_roberta_state())
    cap = {}
    model.text_encoder.register_forward_hook(
        lambda m, i, o: cap.update(hid=o.last_hidden_state.detach(), pool=o.pooler_output.detach()))
    frames = torch.randn(T, 3, H, W, generator=torch.Generator().manual_seed(SEED + 1))
    with torch.no_grad():
        out = model([frames], ["synthetic"], [{"size": torch.tensor((H, W))}])
    assert tuple(cap["hid"].shape) == (1, L, 768), tuple(cap["hid"].shape)
    f32 = lambda t: t.detach().cpu().numpy().astype(np.float32)  # noqa: E731
    fx = {"ids": ids.numpy(), "text_hidden": f32(cap["hid"]), "text_pooled": f32(cap["pool"]),
          "text_seed": np.asarray(TEXT_SEED), "thw": np.asarray([T, H, W]), "frames_seed": np.asarray(SEED + 1),
          "weights_salt": np.asarray(SEED),
          "out_memory_abs_sum": np.asarray(out["memory"].double().abs().sum().item()), "cfg_backbone": np.asarray(BACKBONE)}
    for k in ("pred_logits", "pred_boxes", "pred_masks", "reference_points"):
        fx["out_" + k] = f32(out[k])
    path = os.path.join(HERE, "e2e_swin_t_long_caption.npz")
    np.savez_compressed(path, **fx)
    print("wrote", path, os.path.getsize(path), "bytes; e2e_swin_t_small.npz:",
          os.path.getsize(os.path.join(HERE, "e2e_swin_t_small.npz")))


if __name__ == "__main__":
    main()
