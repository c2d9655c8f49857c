"""CPU: host logic and the C-ABI surface (no compute calls: there is no GPU here)."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    from tce_rvos_amd import build as b
    return b.build(verbose=False)


def _declared(header):
    return set(re.findall(r"\b(tce_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


# header, its symbols spelled out (None: its table is the record), those of them that launch nothing (None: not spelled out; "all":
# every one), its translation units (None: several)
HEADER_CASES = [
    ("tce_rvos.h", None, None, None),
    ("tce_rvos_debug.h", None, "all", None),
    ("tce_rvos_video.h", {"tce_label_objects_u8"}, set(), ("label.hip",)),
    ("tce_rvos_eval.h", {"tce_a2d_masks_u8", "tce_rle_ws_bytes", "tce_rle_counts_u32", "tce_a2d_group_masks_u8"}, {"tce_rle_ws_bytes"},
     ("eval.hip", "a2d_group.hip")),
    ("tce_rvos_score.h", {"tce_jf_ws_bytes", "tce_jf_counts_i32", "tce_rle_decode_ws_bytes", "tce_rle_decode_u8",
                          "tce_mask_overlap_ws_bytes", "tce_mask_overlap_i32"},
     {"tce_jf_ws_bytes", "tce_rle_decode_ws_bytes", "tce_mask_overlap_ws_bytes"}, ("score.hip", "a2d_score.hip")),
    ("tce_rvos_png.h", {"tce_png_stream_bound", "tce_png_ws_bytes", "tce_png_deflate_u8", "tce_png_deflate_dyn_u8"},
     {"tce_png_stream_bound", "tce_png_ws_bytes"}, ("png.hip",)),
    ("tce_rvos_vis.h", {"tce_vis_overlay_u8", "tce_png_filter_rgb_u8", "tce_png_deflate_rows_u8"}, set(), ("vis.hip", "png.hip")),
    ("tce_rvos_pngfile.h", {"tce_png_file_bound", "tce_png_file_ws_bytes", "tce_png_file_u8"},
     {"tce_png_file_bound", "tce_png_file_ws_bytes"}, ("pngfile.hip",)),
    ("tce_rvos_refexp.h", {"tce_refexp_group_u8", "tce_refexp_giou_f32"}, set(), ("refexp.hip",)),
]


@pytest.mark.parametrize("header,symbols,launch_free,source", HEADER_CASES, ids=[c[0] for c in HEADER_CASES])
def test_header_symbols_bound_exported_and_modelled(built_lib, header, symbols, launch_free, source):
    """Every header of include/ against its binding table (_lib.HEADERS), the built library and the hazard checker's tables."""
    from tce_rvos_amd import _lib, hazard
    from tce_rvos_amd import build as b
    assert [c[0] for c in HEADER_CASES] == list(_lib.HEADERS) and set(os.listdir(os.path.join(ROOT, "include"))) == set(_lib.HEADERS)
    assert not [f for f in os.listdir(b.CSRC) if re.fullmatch(r"tce_rvos_.*\.h", f)]  # no entry-point header beside the sources
    table, declared = _lib.HEADERS[header], _declared(header)
    assert declared == set(table), declared ^ set(table)
    assert symbols is None or declared == symbols
    for other, other_table in _lib.HEADERS.items():  # a symbol lives in one header and in one table
        if other != header:
            assert not (declared & set(other_table)) and not (declared & _declared(other)), other
    l, bound = ctypes.CDLL(built_lib), _lib.lib()  # lib() applies the tables
    for name, (res, args) in table.items():
        assert hasattr(l, name), name
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert bound.tce_abi_version() == 5
    # modelled or declared launch-free, never both; the checker's tables hold nothing else
    modelled, free = declared & set(hazard.MODELS), declared & hazard.NOT_LAUNCHES
    assert modelled | free == declared and not (modelled & free), declared - modelled - free
    assert launch_free is None or free == (declared if launch_free == "all" else launch_free)
    every = set().union(*_lib.HEADERS.values())
    assert set(hazard.MODELS) <= every and hazard.NOT_LAUNCHES <= every
    # every object is rebuilt when the header changes, and the stage's translation unit is built
    assert os.path.realpath(os.path.join(ROOT, "include", header)) in {os.path.realpath(d) for d in b.dependencies()}
    assert source is None or all(src in b.SOURCES for src in source)


def test_bad_arguments_are_rejected_with_a_message(built_lib):
    from tce_rvos_amd import _lib
    l = _lib.lib()
    g = _lib.GemmArgs()
    g.M, g.N, g.K = 4, 4, 7  # K not a multiple of 16, null pointers
    assert l.tce_gemm_f32(ctypes.byref(g), None) != 0
    assert b"tce_gemm_f32" in l.tce_last_error()
    assert l.tce_layernorm_f32(None, None, None, None, None, 1, 4, 1e-5, None) != 0
    assert l.tce_msda_fused_f32(None, None, None, None, None, 1, 1, 1, 1, 1, 1, 2, 0, None) != 0


def test_missing_library_fails_loudly(monkeypatch):
    from tce_rvos_amd import _lib
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libtce_rvos.so")
    with pytest.raises(_lib.TceError):
        _lib.lib()


@pytest.mark.parametrize("bb,man", [("swin_t_p4w7", "statedict_swin_t.json"), ("video_swin_t_p4w7", "statedict_vswin_t.json"),
                                    ("resnet50", "statedict_resnet50.json")])
def test_param_manifest_matches_reference_state_dict(bb, man):
    import argparse
    from tce_rvos_amd.config import config_from_args, index_buffers, param_shapes
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", man)))
    cfg = config_from_args(argparse.Namespace(backbone=bb, with_box_refine=True, binary=True, f_token=8, qtrans=True))
    mine = dict(param_shapes(cfg))
    mine.update(index_buffers(cfg))
    for k in list(mine):
        if k.startswith("bbox_embed."):
            mine["transformer.decoder." + k] = mine[k]
    assert set(mine) == set(ref)
    for k, (shape, dtype) in ref.items():
        assert tuple(shape) == tuple(mine[k]), k


def test_model_state_dict_contract_and_build_model_boundary():
    import argparse
    import transformers
    from tce_rvos_amd import build_model
    from tce_rvos_amd.model import ReferFormer
    args = argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True,
                              f_token=8, qtrans=True, num_feature_levels=4, text_encoder_layers=1)
    model, criterion, post = build_model(args)
    assert isinstance(model, ReferFormer)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "statedict_swin_t.json")))
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith("text_encoder.")}
    assert set(sd) == set(ref)
    for k, (shape, dtype) in ref.items():
        assert tuple(sd[k].shape) == tuple(shape) and str(sd[k].dtype).endswith(dtype), k
    # aliasing of the refinement heads (tce_rvos.py:124)
    assert model.transformer.decoder.bbox_embed is model.bbox_embed
    # the reference callers' attribute accesses (main.py:60,63)
    assert model.backbone is not None and model.transformer.encoder is not None
    # strict=False round trip like inference_ytvos.py:150-157
    missing, unexpected = model.load_state_dict({k: v for k, v in model.state_dict().items()}, strict=False)
    assert not missing and not unexpected
    assert all(not p.requires_grad for p in model.text_encoder.parameters())
    with pytest.raises(Exception):
        model([torch.zeros(2, 3, 32, 32)], ["a"], [{"size": torch.tensor([32, 32])}])  # CPU input: no CPU path


def test_vis_loss_state_dict_contract():
    """--vis_loss adds visible_embed.{0..3} (tce_rvos.py:62-63,119-120): same keys and shapes as the reference built with it."""
    import argparse
    from tce_rvos_amd import build_model
    model, _, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, f_token=8, qtrans=True,
                                                 vis_loss=True, contrastive=True, text_encoder_layers=1))
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "statedict_swin_t_vis.json")))
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith("text_encoder.")}
    assert set(sd) == set(ref) and "visible_embed.3.weight" in sd
    assert all(tuple(sd[k].shape) == tuple(ref[k][0]) for k in ref)


def test_plain_flags_state_dict_contract():
    """Without --with_box_refine / --f_token / --qtrans the reference lists its shared heads under every level's
    name and has no frame-token parameters: same keys and shapes here."""
    import argparse
    from tce_rvos_amd import build_model
    model, _, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=False, binary=True, f_token=0,
                                                 qtrans=False, text_encoder_layers=1))
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "statedict_swin_t_plain.json")))
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith("text_encoder.")}
    assert set(sd) == set(ref)
    assert all(tuple(sd[k].shape) == tuple(ref[k][0]) for k in ref)
    assert model.class_embed._modules["3"] is model.class_embed._modules["0"]


def test_unsupported_configs_fail_loudly():
    import argparse
    from tce_rvos_amd import build_model
    with pytest.raises(ValueError):
        build_model(argparse.Namespace(backbone="x3d_m"))
    with pytest.raises(NotImplementedError):
        build_model(argparse.Namespace(backbone="resnet50", dilation=True))
    with pytest.raises(AssertionError):
        build_model(argparse.Namespace(backbone="swin_t_p4w7", two_stage=True))


def test_synth_weights_are_deterministic_and_alias_safe():
    from tce_rvos_amd.weights import synth_tensor
    a = synth_tensor("transformer.decoder.bbox_embed.1.layers.0.weight", (4, 4))
    b = synth_tensor("bbox_embed.1.layers.0.weight", (4, 4))
    assert torch.equal(a, b)
    assert not torch.equal(synth_tensor("x.weight", (4, 4), 0), synth_tensor("x.weight", (4, 4), 1))


def test_nested_tensor_from_videos_list():
    from tce_rvos_amd import nested_tensor_from_videos_list
    nt = nested_tensor_from_videos_list([torch.ones(2, 3, 4, 6), torch.ones(3, 3, 5, 5)])
    assert tuple(nt.tensors.shape) == (2, 3, 3, 5, 6) and tuple(nt.mask.shape) == (2, 3, 5, 6)
    assert not nt.mask[0, :2, :4, :6].any() and nt.mask[0, 2].all() and nt.mask[1, :, :, 5].all()
    # host shape metadata: padded / un-padded is known without reading the mask back from the device
    assert nt.unpadded is False and nt.to("cpu").unpadded is False
    one = nested_tensor_from_videos_list([torch.ones(2, 3, 4, 6)])
    assert one.unpadded is True and not one.mask.any()
    assert nested_tensor_from_videos_list([torch.ones(2, 3, 4, 6)], size_divisibility=4).unpadded is False


def test_arith_override_is_per_thread():
    """per-site arithmetic flips the GEMM mode around groups of launches; the flip must not be visible to another
    host thread issuing (or capturing) launches meanwhile.  ops.arith is a per-thread override of the process default."""
    import threading
    from tce_rvos_amd import ops
    assert ops.get_gemm_mode() == "f16x3"
    seen = {}

    def other():
        seen["mode"] = ops.get_gemm_mode()
        with ops.arith("f32"):
            seen["inner"] = ops.get_gemm_mode()
        seen["after"] = ops.get_gemm_mode()

    with ops.arith("f16"):
        assert ops.get_gemm_mode() == "f16"
        t = threading.Thread(target=other)
        t.start()
        t.join()
        with ops.arith("f16x3"):
            assert ops.get_gemm_mode() == "f16x3"
        assert ops.get_gemm_mode() == "f16"   # nested blocks restore the enclosing override
    assert ops.get_gemm_mode() == "f16x3"
    assert seen == {"mode": "f16x3", "inner": "f32", "after": "f16x3"}
    ops.set_gemm_mode("f16")                  # the process default is what threads without an override see
    try:
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert seen["mode"] == "f16" and seen["after"] == "f16"
    finally:
        ops.set_gemm_mode("f16x3")


def test_ffn_split_plan_is_the_calibrated_one(built_lib):
    """tce_ffn_split_ws_floats / tce_ffn_split_counters (host-side planning, no launch): the hidden-extent split of the fused FFN is
    planned where the measurements say it pays -- launches of 1.1 .. 1.3 rounds of 256 CUs and single partial rounds cut 1 -> 2 or
    2 -> 3 -- and NOT for config 2's 24100-row encoder launches (3 -> 4: measured slower in the clip), full-round launches, other
    widths or GELU."""
    from tce_rvos_amd import _lib
    l = _lib.lib()
    for M, planned in ((24100, False), (72000, False), (192800, False), (85570, False), (18000, True), (40800, True), (16000, True)):
        ws, cnt = l.tce_ffn_split_ws_floats(M, 256, 2048, 1), l.tce_ffn_split_counters(M, 256, 2048, 1)
        if planned:
            assert cnt == (M + 127) // 128 and ws == cnt * 2 * 128 * 256, (M, ws, cnt)
        else:
            assert (ws, cnt) == (0, 0), (M, ws, cnt)
    assert l.tce_ffn_split_ws_floats(18000, 192, 768, 2) == 0 and l.tce_ffn_split_ws_floats(18000, 256, 2048, 2) == 0
    assert l.tce_ffn_split_ws_floats(0, 256, 2048, 1) == 0


def test_bench_dump_outputs_names_dtypes_and_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every tensor of the last step's output dicts becomes <name>.npy in float32 (integers in float64),
    nested results flattened into the name; past the byte budget the largest arrays become fixed seeded samples."""
    import numpy as np
    import bench
    g = torch.Generator().manual_seed(3)
    out = {"pred_masks": torch.randn(1, 2, 3, 40, 50, generator=g), "pred_boxes": torch.rand(1, 2, 3, 4, generator=g).double(),
           "aux_outputs": [{"pred_logits": torch.randn(1, 2, 3, 1, generator=g)}], "idx": torch.arange(5), "ablated": ["x"]}
    bench._dump_outputs(str(tmp_path / "all"), [out])
    got = {f: np.load(tmp_path / "all" / f) for f in sorted(os.listdir(tmp_path / "all"))}
    assert sorted(got) == ["aux_outputs_0_pred_logits.npy", "idx.npy", "pred_boxes.npy", "pred_masks.npy"]
    assert got["pred_masks.npy"].dtype == np.float32 and np.array_equal(got["pred_masks.npy"], out["pred_masks"].numpy())
    assert got["pred_boxes.npy"].dtype == np.float32 and got["idx.npy"].dtype == np.float64
    monkeypatch.setattr(bench, "DUMP_BUDGET", 16 << 20)
    big = {"memory": torch.randn(3 << 20, generator=g), "pred_masks": out["pred_masks"]}
    for d in ("s1", "s2"):
        bench._dump_outputs(str(tmp_path / d), [big, big])
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == ["clip0_memory_sample.npy", "clip0_pred_masks.npy", "clip1_memory_sample.npy", "clip1_pred_masks.npy"]
    s = np.load(tmp_path / "s1" / "clip0_memory_sample.npy")
    assert s.shape == (1 << 20,) and np.isin(s, big["memory"].numpy()).all()
    for f in files:  # the same arguments give the same elements
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f))
