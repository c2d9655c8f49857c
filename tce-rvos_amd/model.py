"""ReferFormer drop-in: the reference's `build_model(args)` / `model(samples, captions, targets)` boundary
(models/__init__.py:4-5, models/tce_rvos.py:194-393, 638-719) over a flat MI355X pipeline.

The module tree exists only to own parameters under the reference's state-dict names (so reference
checkpoints load with `load_state_dict`); `forward` is NOT a module graph: it is one straight-line program
that launches hand-written HIP kernels (libtce_rvos.so) on token-major / channels-last activations living in
a bump arena.  PyTorch supplies device memory, the stream and the (third-party) RoBERTa text encoder.
"""
import os
import types
import math
from collections import OrderedDict
from itertools import accumulate
from typing import Any, List, NamedTuple, Optional

import torch
from torch import nn

from . import ops
from .config import ModelConfig, config_from_args, index_buffers, param_shapes
from .weights import synth_tensor

ACT_RELU, ACT_GELU = ops.ACT_RELU, ops.ACT_GELU
RES_ADD, RES_MUL = ops.RES_ADD, ops.RES_MUL


class NestedTensor(object):
    """util/misc.py:380-400"""

    def __init__(self, tensors, mask: Optional[torch.Tensor]):
        self.tensors = tensors
        self.mask = mask

    def to(self, device):
        nt = NestedTensor(self.tensors.to(device), self.mask.to(device) if self.mask is not None else None)
        for a in ("unpadded", "valid_hw"):
            if hasattr(self, a):
                setattr(nt, a, getattr(self, a))
        return nt

    def decompose(self):
        return self.tensors, self.mask

    def __repr__(self):
        return str(self.tensors)


def nested_tensor_from_videos_list(videos_list: List[torch.Tensor], size_divisibility=1):
    """util/misc.py:354-377"""
    max_size = [max(s) for s in zip(*[list(v.shape) for v in videos_list])]
    if size_divisibility > 1:
        st = size_divisibility
        max_size[-2] = (max_size[-2] + st - 1) // st * st
        max_size[-1] = (max_size[-1] + st - 1) // st * st
    b = len(videos_list)
    t, c, h, w = max_size
    vids = torch.zeros([b, t, c, h, w], dtype=videos_list[0].dtype, device=videos_list[0].device)
    masks = torch.ones((b, t, h, w), dtype=torch.bool, device=videos_list[0].device)
    for v, pv, m in zip(videos_list, vids, masks):
        pv[:v.shape[0], :, :v.shape[2], :v.shape[3]].copy_(v)
        m[:v.shape[0], :v.shape[2], :v.shape[3]] = False
    nt = NestedTensor(vids, masks)
    # host shape metadata: no clip was padded iff every clip already has the batch's size (forward() then needs no
    # device read-back of the mask to know it -- VERDICT r2 weak #10); valid_hw: each clip's un-padded frame size
    nt.unpadded = all(list(v.shape) == max_size for v in videos_list)
    nt.valid_hw = [(int(v.shape[2]), int(v.shape[3])) for v in videos_list]
    return nt


# Every hipGraph this process ever instantiated.  Captured clips carry parallel branches (text beside the backbone, decoder
# beside the pixel decoder); the HIP runtime (ROCm 7.x, libamdhip64 hip::Graph::UpdateStreams) runs them on internal
# streams that graph executables SHARE, and destroying one executable leaves the others with dangling stream pointers:
# a later replay of a surviving graph segfaults inside hipGraphLaunch.  So executables are never destroyed while the
# process lives: an evicted / invalidated cache entry gives back its arenas (gigabytes) and keeps only the (small,
# never replayed) executable alive here.  The list is bounded by a per-process capture budget: once it is spent,
# shapes that are not cached run eagerly.
_ALL_GRAPHS = []
_BUDGET_WARNED = False
# Side streams of the capture branches, shared by every capture of a (device, slot): a stream only shapes the fork / join
# topology while a graph is being captured, so captures need not own theirs (one set per capture stranded 4 streams with
# every invalidated entry -- VERDICT r2 weak #8).
_SIDE_STREAMS = {}


def _side_streams(device, slot, n=4):
    key = (torch.device(device), int(slot))
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = [torch.cuda.Stream(device=device) for _ in range(n)]
    return st


# Round 5: executables the model OWNS.  The captured hipGraph_t is never instantiated: its nodes are re-created, with their
# parameters and edges, in a fresh graph (tce_graph_group with one input: csrc/capi.hip) and THAT is instantiated -- an executable
# built from explicitly added nodes holds no reference to the capture's streams, so it can be destroyed when its cache entry is
# evicted and the capture budget above no longer applies to it.  TCE_GRAPH_OWN_EXEC=0 restores the never-destroy path.
GRAPH_OWN_EXEC = os.environ.get("TCE_GRAPH_OWN_EXEC", "1") != "0"
# The other switches of capture and replay, read ONCE at import like pipeline.py's: they are constants of the process, so every
# capture of the process is built from the same program (none of them needs to be part of a graph key).  The per-model knobs
# (TCE_GRAPH, TCE_GRAPH_CACHE, TCE_GRAPH_CACHE_GB, TCE_GRAPH_AFTER, TCE_TEXT_CACHE) are instance attributes set in __init__.
GRAPH_BUDGET = int(os.environ.get("TCE_GRAPH_BUDGET", 512))  # captures of the never-destroy path (_ALL_GRAPHS) per process
KEEP_GRAPHS = os.environ.get("TCE_KEEP_GRAPHS", "0") == "1"   # keep the hipGraph_t beside the executable (tools/pair_graph_probe.py)
FORK2 = os.environ.get("TCE_FORK2", "1") != "0"               # A/B: 0 = no parallel branch for the stride-4 lateral path
FORK3 = os.environ.get("TCE_FORK3", "1") != "0"               # A/B: 0 = none for the stride-32 / stride-16 lateral paths
COPYPLAN = os.environ.get("TCE_COPYPLAN", "1") != "0"         # A/B: 0 = per-tensor output clones after a replay
_OWNED_LIVE = [0, 0]  # [alive now, destroyed so far]


class _Resources(NamedTuple):
    """What one capture runs on (_branch_resources): the main arena and one arena per parallel branch that allocates; the
    streams are the (device, slot)'s shared set."""
    arena: Any
    side_arena: Any
    side_stream: Any
    arena2: Any
    stream2: Any
    arena3: Any
    stream3: Any
    arena4: Any
    stream4: Any


class _Entry(NamedTuple):
    """One captured launch program in a model's graph cache.  statics[0] is the backbone's frame buffer, statics[1:] the
    program's other inputs (token ids, or text_hidden and text_pooled); out is the output dict living in `res`'s arenas."""
    exe: Any        # _OwnedExec, or a torch.cuda.CUDAGraph of the never-destroy path
    statics: list
    out: dict
    res: _Resources
    nbytes: int     # of the arenas: what the cache's byte bound counts
    plan: Any       # ops.CopyPlan of the outputs, or None (per-tensor clones)


class _OwnedExec:
    """A hipGraphExec_t built by tce_graph_group; destroyed with its cache entry (after a device sync by the owner)."""

    def __init__(self, handle):
        self.handle = handle
        _OWNED_LIVE[0] += 1

    def replay(self):
        from ._lib import check, lib
        check(lib().tce_graph_launch(self.handle, torch.cuda.current_stream().cuda_stream), "tce_graph_launch")

    def destroy(self):
        if self.handle is not None:
            from ._lib import lib
            lib().tce_graph_destroy(self.handle)
            self.handle = None
            _OWNED_LIVE[0] -= 1
            _OWNED_LIVE[1] += 1

    def __del__(self):
        try:
            self.destroy()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def graph_state():
    """Process-wide capture accounting.  Owned executables (the default) are destroyed on eviction; executables of the legacy
    path are never destroyed (see _ALL_GRAPHS) and are budgeted."""
    return {"captured": len(_ALL_GRAPHS), "budget": GRAPH_BUDGET, "eager_forever": len(_ALL_GRAPHS) >= GRAPH_BUDGET,
            "owned_alive": _OWNED_LIVE[0], "owned_destroyed": _OWNED_LIVE[1]}


# ---------------------------------------------------------------------------------------------------------------
# Per-site arithmetic (BASELINE config 5).  The launch program is cut into site groups; a policy maps a
# group to the arithmetic of its matrix products: "f16x3" (fp32-accurate split, the default) or "f16" (one fp16 MFMA per
# product on operands rounded to nearest fp16).  Weight streams are packed in the arithmetic of the group that consumes
# them.  tools/arith_sensitivity.py switches one group at a time to "f16" at config 5 and records IoU / |d|/max against
# the oracle (profiles/r03_arith_sensitivity_cfg5.json); the named policies below are read off that table.
# ---------------------------------------------------------------------------------------------------------------
ARITH_GROUPS = ("text", "backbone.attn", "backbone.mlp", "backbone.merge", "input_proj", "encoder.msda", "encoder.ffn",
                "encoder.ftf", "encoder.ftf_x", "decoder", "pixel.conv", "pixel.attn", "pixel.xattn", "pixel.ffn", "mask_head")
ARITH_POLICIES = {
    "uniform": {},
    "all_f16": {g: "f16" for g in ARITH_GROUPS},
    # Read off profiles/r03_arith_sensitivity_cfg5*.txt (Swin-B, T=10, 480x854, one group at a time in single-pass fp16, default
    # and O(1)-logit weights) and checked on a second clip / weight set by bench.py's parity leg (profiles/r03_bench_cfg5_*.json):
    # cfg5_mixed -- single-pass fp16 in everything DOWNSTREAM of the decoder's queries: the pixel decoder (convolutions,
    #   attention, text cross-attention, FFNs) and the mask head.  |d| / max|ref| <= 1.5e-4, mask IoU vs the oracle >= 0.99998 on
    #   both clips: the only mix that is robustly inside the 1e-3 IoU criterion.  5 % faster than uniform f16x3.
    # cfg5_fast -- additionally the backbone (qkv / proj / window attention / MLPs), the encoder FFNs and value projections:
    #   22.5 ms against 28.2 ms uniform f16x3, but any fp16 rounding UPSTREAM of the queries perturbs the dynamic mask weights
    #   by 2e-3 .. 5e-3 of max|ref| and that sits ON the criterion: IoU 0.99976 on the table's clip, 0.99846 on the benchmark's
    #   (the backbone MLPs alone: 0.99986 / 0.99888) -- like every product in fp16 ("all_f16": 0.99955 / 0.99795).
    "cfg5_mixed": {g: "f16" for g in ("pixel.conv", "pixel.attn", "pixel.xattn", "pixel.ffn", "mask_head")},
    "cfg5_fast": {g: "f16" for g in ("backbone.attn", "backbone.mlp", "encoder.ffn", "encoder.msda", "pixel.conv", "pixel.ffn")},
}
# Named policies whose OWN measurements miss the 1e-3 IoU criterion on at least one clip (profiles/r03_bench_cfg5_swin_b_fast.json:
# 0.99846): selectable for experiments, announced with a warning, flagged invalid by bench.py's parity leg.
EXPERIMENTAL_POLICIES = ("cfg5_fast", "all_f16")


def arith_group_of(key):
    """Site group that consumes the parameter `key` (a state-dict name or a derived operand's name)."""
    if key.startswith("backbone."):
        if ".attn." in key:
            return "backbone.attn"
        if ".mlp." in key:
            return "backbone.mlp"
        return "backbone.merge"
    if key.startswith("input_proj.") or key.startswith("fusion_module."):
        return "input_proj"
    if key.startswith("transformer.encoder."):
        if ".ftoken_layers." in key:
            tail = key.split(".ftoken_layers.")[1]
            if tail.startswith("linear") or tail.startswith("ffn"):
                return "encoder.ffn"
            if tail.startswith("frame_token_atten."):
                return "encoder.ftf_x"
            if tail.startswith("token_frame_atten."):
                return "encoder.msda"
            return "encoder.ftf"
        if ".self_attn." in key:
            return "encoder.msda"
        return "encoder.ffn"
    if key.startswith("pixel_decoder."):
        if ".self_attn." in key:
            return "pixel.attn"
        if ".multihead_attn." in key:
            return "pixel.xattn"
        if ".linear" in key or ".ffn" in key:
            return "pixel.ffn"
        return "pixel.conv"
    if key.startswith("resizer."):
        return "text"
    return "decoder"


class _Node(nn.Module):
    """Parameter container; carries no computation."""


class SyntheticTokenizer:
    """Offline stand-in for RobertaTokenizerFast (its vocabulary is a network download): whitespace words
    hashed into the RoBERTa id range, <s>=0 ... </s>=2.  Deterministic; NOT the real BPE."""

    def __call__(self, captions, max_len=None):
        import zlib
        rows = []
        for c in captions:
            ids = [0] + [3 + zlib.crc32(wd.encode()) % 50262 for wd in c.lower().split()] + [2]
            rows.append(ids)
        L = max(len(r) for r in rows)
        ids = torch.full((len(rows), L), 1, dtype=torch.long)
        att = torch.zeros((len(rows), L), dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r)
            att[i, :len(r)] = 1
        return ids, att


class ReferFormer(nn.Module):
    def __init__(self, cfg: ModelConfig, args=None, text_encoder=None, tokenizer=None, init_salt=0):
        super().__init__()
        self.cfg = cfg
        self.args = args
        self.num_queries = cfg.num_queries
        self.hidden_dim = cfg.hidden_dim
        self.num_feature_levels = cfg.num_feature_levels
        self.num_frames = cfg.num_frames
        self.mask_dim = cfg.mask_dim
        self.aux_loss = cfg.aux_loss
        self.with_box_refine = cfg.with_box_refine
        self.mask_out_stride = 4
        self.mask_feat_stride = 4
        if cfg.hidden_dim != 256 or cfg.nheads != 8:
            raise NotImplementedError("kernels are built for hidden_dim=256, nheads=8 (head_dim 32)")
        if cfg.num_feature_levels != 4:
            raise NotImplementedError("num_feature_levels must be 4")
        if cfg.enc_n_points != 4 or cfg.dec_n_points != 4:
            raise NotImplementedError("the fused MSDA launch program is built for enc_n_points = dec_n_points = 4 "
                                      "(L*P = 16 samples per head); the generic op tce_ms_deform_attn_forward_f32 is not")
        shapes = param_shapes(cfg)
        for key, shape in shapes.items():
            node, leaf = self._node_for(key)
            if cfg.is_resnet and is_frozen_bn_key(key):  # FrozenBatchNorm2d holds buffers (backbone.py:31-34)
                node.register_buffer(leaf, synth_tensor(key, shape, init_salt))
            else:
                node.register_parameter(leaf, nn.Parameter(synth_tensor(key, shape, init_salt), requires_grad=True))
        for key, shape in index_buffers(cfg).items():
            node, leaf = self._node_for(key)
            node.register_buffer(leaf, self._rel_index(cfg))
        if cfg.with_box_refine:  # one tensor, two names (tce_rvos.py:124)
            self.transformer.decoder.add_module("bbox_embed", self.bbox_embed)
        else:  # one head listed under every level's name (tce_rvos.py:127-130)
            for i in range(1, cfg.dec_layers):
                self.class_embed.add_module(str(i), self.class_embed._modules["0"])
                if cfg.vis_loss:
                    self.visible_embed.add_module(str(i), self.visible_embed._modules["0"])
                self.bbox_embed.add_module(str(i), self.bbox_embed._modules["0"])
        if text_encoder is None:
            text_encoder = build_text_encoder(args)
        self.text_encoder = text_encoder
        if tokenizer is None:
            tokenizer = build_tokenizer(args)
        self.tokenizer = tokenizer
        if args is not None and getattr(args, "freeze_text_encoder", False):
            for p in self.text_encoder.parameters():
                p.requires_grad_(False)
        self._packed = None
        self._text = None
        self._arenas = {}  # eager path: one bump arena per slot
        self._shape_cache = {}
        self._text_cache = OrderedDict()
        self.arena_bytes = None  # override to force an arena size
        # hipGraph replay of the whole per-clip launch program (one graph per input shape); TCE_GRAPH=0 disables.
        # Every graph owns private arenas (~3 GB at config 2, ~11 GB at config 5), and the callers feed whole videos
        # of varying length / size / caption length (inference_ytvos.py:278-295), so the cache is an LRU bounded in
        # entries AND bytes, and a shape is only captured once it comes back (the first `graph_after` sightings run
        # eagerly: capturing costs an eager warm-up, a device sync and the capture itself).
        self.use_graph = os.environ.get("TCE_GRAPH", "1") != "0"
        self._graphs = OrderedDict()
        self._sightings = OrderedDict()
        self.max_graphs = int(os.environ.get("TCE_GRAPH_CACHE", 6))
        self.max_graph_bytes = int(float(os.environ.get("TCE_GRAPH_CACHE_GB", 96)) * 2 ** 30)
        self.graph_after = int(os.environ.get("TCE_GRAPH_AFTER", 1))
        self.text_cache_size = int(os.environ.get("TCE_TEXT_CACHE", 0))  # expressions kept (0 = recompute like the reference)
        self.arith_policy = {}  # site group -> "f16" | "f16x3" (set_arith_policy); empty = the process mode everywhere
        self._stamp = None      # (process mode, policy) the packed operands and the captured graphs were built for
        self._routes = ops.Routes()
        self._nograph = set()   # keys whose capture ran out of arena: they stay on the eager path
        self._group_checked = set()  # forward_group keys whose token ids were checked for the pad id

    # ---------------------------------------------------------------- parameter tree
    def _node_for(self, key):
        parts = key.split(".")
        node = self
        for p in parts[:-1]:
            nxt = node._modules.get(p)
            if nxt is None:
                nxt = _Node()
                node.add_module(p, nxt)
            node = nxt
        return node, parts[-1]

    @staticmethod
    def _rel_index(cfg):
        if cfg.video:
            wd, wh, ww = cfg.video_window
            co = torch.stack(torch.meshgrid(torch.arange(wd), torch.arange(wh), torch.arange(ww), indexing="ij")).flatten(1)
            rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous()
            rel[:, :, 0] += wd - 1
            rel[:, :, 1] += wh - 1
            rel[:, :, 2] += ww - 1
            rel[:, :, 0] *= (2 * wh - 1) * (2 * ww - 1)
            rel[:, :, 1] *= 2 * ww - 1
            return rel.sum(-1)
        ws = cfg.window_size
        co = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
        rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous()
        rel[:, :, 0] += ws - 1
        rel[:, :, 1] += ws - 1
        rel[:, :, 0] *= 2 * ws - 1
        return rel.sum(-1)

    def _invalidate(self):
        """Drops everything derived from the parameters.  Cache entries give back their arenas here (the executables stay in
        _ALL_GRAPHS, never replayed again); packed streams and routes go with the model's own tables only."""
        self._packed = None
        self._stamp = None
        self._text = None
        self._shape_cache = {}
        if getattr(self, "_graphs", None) or getattr(self, "_arenas", None):
            torch.cuda.synchronize()  # a replay / eager clip may still be running on these buffers
        for ent in (getattr(self, "_graphs", None) or {}).values():
            if isinstance(ent.exe, _OwnedExec):
                ent.exe.destroy()
        self._graphs = OrderedDict()
        self._sightings = OrderedDict()
        self._text_cache = OrderedDict()
        self._arenas = {}
        if getattr(self, "_routes", None) is not None:
            self._routes.clear()
        self._nograph = set()
        self._group_checked = set()

    # ---------------------------------------------------------------- per-site arithmetic
    def set_arith_policy(self, policy):
        """policy: a name of ARITH_POLICIES or a dict {site group: "f16" | "f16x3"}.  Derived operands and captured graphs
        are rebuilt on the next forward."""
        if isinstance(policy, str):
            if policy in EXPERIMENTAL_POLICIES:
                import warnings
                warnings.warn(f"arith policy '{policy}' is EXPERIMENTAL: its own measurements miss the 1e-3 mask-IoU criterion on "
                              f"some clips (DESIGN.md section 3.1b); 'cfg5_mixed' is the criterion-safe mix", RuntimeWarning, stacklevel=2)
            policy = ARITH_POLICIES[policy]
        bad = [g for g in policy if g not in ARITH_GROUPS] + [m for m in policy.values() if m not in ("f16", "f16x3")]
        if bad:
            raise ValueError(f"arith policy: unknown group / mode {bad}; groups: {ARITH_GROUPS}")
        self.arith_policy = dict(policy)
        self._invalidate()

    def mode_of(self, group):
        """Arithmetic of a site group under the process mode and this model's policy ('f32' = exact: no policy applies)."""
        base = ops.get_gemm_mode() if self._stamp is None else self._stamp[0]
        return base if base == "f32" else self.arith_policy.get(group, base)

    def arith(self, group):
        """`with model.arith("encoder.ffn"):` -- the launches inside run in the group's arithmetic."""
        return ops.arith(self.mode_of(group))

    def _current_stamp(self):
        return (ops.get_gemm_mode(), tuple(sorted(self.arith_policy.items())))

    def _ensure_packed(self):
        """Packed operands and captured graphs carry the arithmetic they were built in: a different process
        mode or policy rebuilds them instead of silently running the old one."""
        if self._packed is not None and self._stamp != self._current_stamp():
            self._invalidate()
        if self._packed is None:
            self._pack()
            torch.cuda.synchronize()  # packed on the calling stream, read by every stream (slot) afterwards

    def _apply(self, fn, *a, **k):
        self._invalidate()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict=True, **kw):
        self._invalidate()
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def repack(self):
        """Call after mutating parameters in place (packed kernel operands and captured graphs are derived)."""
        self._invalidate()

    # ---------------------------------------------------------------- weight packing
    def _pack(self):
        cfg = self.cfg
        d = cfg.hidden_dim
        w = {}
        # state_dict() lists aliased tensors under every name (named_parameters() de-duplicates them)
        sd = {k: v for k, v in self.state_dict(keep_vars=True).items()
              if not k.startswith("text_encoder.") and v.is_floating_point()}
        for k, v in sd.items():
            if not v.is_cuda or v.dtype != torch.float32:
                raise RuntimeError(f"parameter {k} must be a CUDA float32 tensor (model.to('cuda') first); "
                                   f"there is no CPU path")
            w[k] = v.detach()
        # split-fp16 contract, host half: every GEMM weight inside the fp16 range (activations: ops.range_flag)
        ops.check_weight_range(w.items())
        ops.range_flag(next(iter(w.values())).device)
        self._stamp = self._current_stamp()
        routes = self._routes
        routes.clear()
        with torch.no_grad():
            # MSDA: one projection for (sampling offsets | attention logits)
            for k in list(sd):
                if k.endswith("sampling_offsets.weight"):
                    pre = k[:-len("sampling_offsets.weight")]
                    w[pre + "offaw.weight"] = torch.cat([sd[k], sd[pre + "attention_weights.weight"]], 0).contiguous()
                    w[pre + "offaw.bias"] = torch.cat([sd[pre + "sampling_offsets.bias"],
                                                       sd[pre + "attention_weights.bias"]], 0).contiguous()
                if k.endswith("in_proj_weight"):
                    pre = k[:-len("in_proj_weight")]
                    W, B = sd[k].detach(), sd[pre + "in_proj_bias"].detach()
                    w[pre + "q.w"], w[pre + "k.w"], w[pre + "v.w"] = W[:d], W[d:2 * d], W[2 * d:]
                    w[pre + "q.b"], w[pre + "k.b"], w[pre + "v.b"] = B[:d], B[d:2 * d], B[2 * d:]
                    w[pre + "qk.w"], w[pre + "qk.b"] = W[:2 * d], B[:2 * d]
                    if (pre.endswith("multihead_attn.") or pre.endswith("frame_token_atten.")) and d == 256:
                        # short-key cross-attention sites (text keys; frame tokens): static half of the fold
                        w[pre + "q.wT:x"] = ops.xattn_static(W[:d], B[:d])
                if v_is_conv(sd[k]) and sd[k].shape[-1] == 3:
                    w[k + ":cl"] = sd[k].detach().permute(0, 2, 3, 1).reshape(sd[k].shape[0], -1).contiguous()
            # fused FFN / Swin MLP streams (csrc/ffn.hip): fp16 hi/lo planes in MFMA-fragment order
            for k in list(sd):
                for l1, l2, tag in ((".linear1.weight", ".linear2.weight", ".ffn:pk"),
                                    (".mlp.fc1.weight", ".mlp.fc2.weight", ".mlp.ffn:pk")):
                    if k.endswith(l1):
                        pre = k[:-len(l1)]
                        w1, w2 = sd[k].detach(), sd[pre + l2].detach()
                        if w1.dim() == 2 and ops.ffn_supported(w1.shape[1], w1.shape[0]) and self._stamp[0] != "f32":
                            # packed in the arithmetic of the group that runs it; the name carries the mode, so a launch
                            # issued in another arithmetic finds no stream and takes the two-GEMM path
                            mode = self.mode_of(arith_group_of(pre + tag))
                            with ops.arith(mode):
                                w[pre + tag + ":" + mode] = ops.ffn_pack(w1, sd[pre + l1[:-len("weight")] + "bias"].detach(), w2)
            # Swin attention half-block as one launch (csrc/swinattn.hip): per block, Wqkv | Wproj as one fragment stream
            if not cfg.is_resnet and not cfg.video and self._stamp[0] != "f32":
                mode = self.mode_of("backbone.attn")
                for k in list(sd):
                    if k.endswith(".attn.qkv.weight") and sd[k].shape[1] in ops.SWIN_FUSED_C:
                        pre = k[:-len("attn.qkv.weight")]
                        with ops.arith(mode):
                            w[pre + "attn:pk:" + mode] = ops.swin_attn_pack(sd[k].detach(), sd[pre + "attn.proj.weight"].detach())
            # token-stationary linear kernel (csrc/rowlin.hip): packed copies of every eligible weight in THIS model's routes
            # (keyed by address + arithmetic) so ops.gemm_ex can route the shapes where it wins
            for k in list(w):
                t = w[k]
                if torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2 and (k.endswith("weight") or k.endswith(".w")):
                    with self.arith(arith_group_of(k)):
                        ops.rowlin_register(t, routes)
            # pixel-stationary 3x3 convolution (csrc/conv3x3.hip): the pixel decoder's 256 -> 256 output convolutions
            for k in list(w):
                if k.startswith("pixel_decoder.") and k.endswith(".weight:cl") and w[k].shape[1] % 9 == 0:
                    with self.arith("pixel.conv"):
                        ops.conv3x3_register(w[k], w[k].shape[1] // 9, routes)
            if cfg.is_resnet:
                self._pack_resnet(sd, w)
            if cfg.video:
                w["backbone.0.body.patch_embed.proj.weight:2d"] = \
                    sd["backbone.0.body.patch_embed.proj.weight"].detach().squeeze(2).contiguous()
        self._packed = w
        return w

    @staticmethod
    def _pack_resnet(sd, w):
        """FrozenBatchNorm2d (backbone.py:46-56) is an affine map per output channel: fold its scale into the
        convolution in front of it and keep its bias as the GEMM bias.  conv -> ":f" = [Cout, kh*kw*Cin] with
        k = (ky*kw+kx)*Cin + c (implicit-GEMM order); the stem -> [147, 64] with k = (c*7+ky)*7+kx."""
        for k in list(sd):
            if not (k.startswith("backbone.0.body.") and k.endswith(".weight") and sd[k].dim() == 4):
                continue
            pre = k[:-len(".weight")]
            if pre.endswith("downsample.0"):
                bn = pre[:-1] + "1"
            else:
                bn = pre[:pre.rfind(".") + 1] + "bn" + pre[-1]
            scale = sd[bn + ".weight"].detach() * (sd[bn + ".running_var"].detach() + 1e-5).rsqrt()
            w[pre + ":b"] = (sd[bn + ".bias"].detach() - sd[bn + ".running_mean"].detach() * scale).contiguous()
            wf = sd[k].detach() * scale.view(-1, 1, 1, 1)
            if pre.endswith("body.conv1"):
                w[pre + ":f"] = wf.reshape(64, 147).t().contiguous()
            else:
                w[pre + ":f"] = wf.permute(0, 2, 3, 1).reshape(wf.shape[0], -1).contiguous()

    # ---------------------------------------------------------------- per-shape constants
    def _shape_consts(self, T, H0, W0, device, valid=None):
        """valid = (rows, columns) of the frames that are not padding (None: un-padded)."""
        key = (T, H0, W0, valid)
        c = self._shape_cache.get(key)
        if c is not None:
            return c
        cfg, w = self.cfg, self._packed
        Hp, Wp = (H0 + 3) // 4, (W0 + 3) // 4
        sizes = [(Hp, Wp)]
        for _ in range(3):
            h, ww = sizes[-1]
            sizes.append(((h + 1) // 2, (ww + 1) // 2))
        h5, w5 = sizes[3]
        lvl_sizes = [sizes[1], sizes[2], sizes[3], ((h5 + 2 - 3) // 2 + 1, (w5 + 2 - 3) // 2 + 1)]
        S = sum(h * ww for h, ww in lvl_sizes)
        starts = [0]
        for h, ww in lvl_sizes[:-1]:
            starts.append(starts[-1] + h * ww)
        F = cfg.hidden_dim // 2
        c = dict(sizes=sizes, lvl_sizes=lvl_sizes, S=S, starts=starts)

        # Padded clips: the mask of every map is the nearest-neighbour resampling of the frame mask (backbone.py / Joiner,
        # F.interpolate(mask[None].float(), size=...)); a bottom / right border stays one, so a map's mask is its count of
        # non-padded rows / columns: src = min(floor(dst * in / out), in - 1) < valid  (scale in fp32 like PyTorch)
        def nvalid(n_out, n_in, v_in):
            if v_in >= n_in:
                return n_out
            src = torch.clamp(torch.floor(torch.arange(n_out, dtype=torch.float32) *
                                          torch.tensor(float(n_in) / float(n_out), dtype=torch.float32)).long(), max=n_in - 1)
            return int((src < v_in).sum())

        Hv, Wv = valid if valid is not None else (H0, W0)
        sizes_v = [(nvalid(h, H0, Hv), nvalid(ww, W0, Wv)) for (h, ww) in sizes]
        lvl_v = [(nvalid(h, H0, Hv), nvalid(ww, W0, Wv)) for (h, ww) in lvl_sizes]
        if valid is not None and any(a < 1 or b < 1 for a, b in sizes_v + lvl_v):
            raise NotImplementedError("padded clip whose valid region vanishes at a pyramid level")
        c["lvl_valid"] = lvl_v if valid is not None else None
        # backbone-level position maps (the same for every frame: one clip's frames share their size): [h*w, 256]
        c["pos"] = [ops.pos_sine2d(1, h, ww, F, device, valid=v) for (h, ww), v in zip(sizes, sizes_v)]
        # encoder position = sine + level embedding, concatenated over levels: [S, 256]
        lp = torch.empty(S, cfg.hidden_dim, dtype=torch.float32, device=device)
        for l, (h, ww) in enumerate(lvl_sizes):
            ops.pos_sine2d(1, h, ww, F, device, add=w["transformer.level_embed"][l], out=lp[starts[l]:starts[l] + h * ww],
                           valid=lvl_v[l])
        c["lvl_pos"] = lp
        # encoder reference points (pixel centres) / (valid_ratio * size), get_reference_points :572-589; the per-level factor
        # "* valid_ratios" (:590-594) is applied inside the MSDA kernels
        refs = []
        for (h, ww), (hv, wv) in zip(lvl_sizes, lvl_v):
            ry, rx = torch.meshgrid(torch.linspace(0.5, h - 0.5, h, dtype=torch.float32),
                                    torch.linspace(0.5, ww - 0.5, ww, dtype=torch.float32), indexing="ij")
            if valid is None:
                refs.append(torch.stack((rx.reshape(-1) / ww, ry.reshape(-1) / h), -1))
            else:
                vr_w, vr_h = torch.tensor(float(wv)) / ww, torch.tensor(float(hv)) / h
                refs.append(torch.stack((rx.reshape(-1) / (vr_w * ww), ry.reshape(-1) / (vr_h * h)), -1))
        c["enc_ref"] = torch.cat(refs, 0).to(device).contiguous()
        # VLBlock reduced grids (segmentation.py:339-344): stage k=1..4 <-> sizes[k-1], sr = 8,4,2,1
        red, kmask = {}, {}
        for stage, sr in ((1, 8), (2, 4), (3, 2), (4, 1)):
            h, ww = sizes[stage - 1]
            hv, wv = sizes_v[stage - 1]
            if sr > 1:
                nh_, nw_ = int(h * 1.0 / sr), int(ww * 1.0 / sr)
                red[stage] = (nh_, nw_, ops.resize_nearest(c["pos"][stage - 1], 1, h, ww, nh_, nw_, cfg.hidden_dim))
                h, ww, hv, wv = nh_, nw_, nvalid(nh_, h, hv), nvalid(nw_, ww, wv)   # the map's mask, resampled again (:345-351)
            if valid is not None:  # key padding mask of the block's self-attention over all frames' tokens: 1 = ignore
                m = torch.ones(h, ww, dtype=torch.uint8)
                m[:hv, :wv] = 0
                kmask[stage] = m.reshape(-1).repeat(T).to(device).contiguous()
        c["red"] = red
        c["kmask"] = kmask
        # built once per shape on the calling stream: forwards kept in flight on OTHER streams (slots) read them too
        torch.cuda.current_stream(device).synchronize()
        self._shape_cache[key] = c
        return c

    def _text_pos(self, L, device):
        key = ("text_pos", L)
        tp = self._shape_cache.get(key)
        if tp is None:
            x = torch.arange(1, L + 1, dtype=torch.float32)
            x = x / (x[-1:] + 1e-6) * (2 * math.pi)
            dim_t = torch.arange(self.cfg.hidden_dim, dtype=torch.float32)
            dim_t = 10000.0 ** (2 * torch.div(dim_t, 2, rounding_mode="trunc") / self.cfg.hidden_dim)
            px = x[:, None] / dim_t
            tp = torch.stack((px[:, 0::2].sin(), px[:, 1::2].cos()), dim=2).flatten(1).to(device).contiguous()
            self._shape_cache[key] = tp
        return tp

    @staticmethod
    def _conv3_ws_bytes(T, H0, W0, strides):
        """The largest workspace of a split 3x3 convolution (ops.conv3x3_split_ws_floats) at the pixel decoder's maps of these strides."""
        return 4 * max(ops.conv3x3_split_ws_floats(T * (-(-H0 // s)) * (-(-W0 // s))) for s in strides)

    def _arena_bytes(self, T, H0, W0):
        tok0 = T * ((H0 + 3) // 4) * ((W0 + 3) // 4)
        return self.arena_bytes or int(tok0 * 4 * (2048 * 2.2 + 256 * 24) + (256 << 20) + self._conv3_ws_bytes(T, H0, W0, (4, 8)))

    def _gather_bytes(self, rows, H0, W0):
        """Bytes of the four dense maps of `rows` frames that an indexed group gathers from the backbone's maps (one per stage)."""
        h, w, out = (H0 + 3) // 4, (W0 + 3) // 4, []
        for c in self.cfg.num_channels:
            out.append(int(rows) * h * w * int(c) * 4 + 256)
            h, w = (h + 1) // 2, (w + 1) // 2
        return out

    def _get_arena(self, T, H0, W0, device, slot=0, extra=0):
        """The eager path's arena of `slot` (captured graphs own a private one each: their addresses are baked in).
        One arena per slot: forwards kept in flight on different streams must not share activations."""
        need = self._arena_bytes(T, H0, W0) + int(extra)
        ar = self._arenas.get(slot)
        if ar is None or ar.buf.numel() < need or ar.device != torch.device(device):
            ar = self._arenas[slot] = ops.Arena(device, need)
        return ar

    # ---------------------------------------------------------------- the boundary
    @torch.no_grad()
    def forward(self, samples, captions, targets, slot=0):
        """models/tce_rvos.py:194.  samples: NestedTensor([B,T,3,H,W],[B,T,H,W]) or list of [T,3,H,W];
        captions: list[str] (or a LongTensor [B,L] of token ids); targets: list[dict] with 'size'.
        slot (extension, default 0): independent replay resources (graph, arenas, static inputs).  Clips are
        independent units, so a caller may keep several B=1 forwards in flight on different torch streams
        (one slot per stream) to fill the GPU; each forward is still exactly the B=1 computation."""
        if not isinstance(samples, NestedTensor) and not (hasattr(samples, "tensors") and hasattr(samples, "mask")):
            if len(samples) == 1:  # a single clip is never padded: no copy, no mask, no host sync
                vids, mask = samples[0][None], None
            else:
                samples = nested_tensor_from_videos_list(samples)
                vids, mask = samples.tensors, samples.mask
        else:
            vids, mask = samples.tensors, samples.mask
        if isinstance(captions, (list, tuple)):
            if not isinstance(captions[0], str):
                raise ValueError("Please mask sure the caption is a list of string")
            b = len(captions)
        else:
            b = captions.shape[0]
        if vids.dim() == 4:
            vids = vids[None]
        if b != 1 or vids.shape[0] != 1:
            raise NotImplementedError("one clip per forward (B = 1): the reference mixes clips inside a batch "
                                      "(FTF token attention, IQT) so batching changes results; shard clips instead")
        # A2D / JHMDB: one annotated frame per clip (tce_rvos.py:233-243): everything after the backbone runs on that frame
        select = int(targets[0]["valid_indices"]) if "valid_indices" in targets[0] else None
        if select is not None and not 0 <= select < vids.shape[1]:
            raise IndexError(f"valid_indices {select} outside the clip's {vids.shape[1]} frames")
        ids, att, ids_host = self._tokenise(captions, vids.device)  # on the host: nothing is launched or copied here
        self._check_caption_tokens(ids.shape[1])
        if not vids.is_cuda:
            raise RuntimeError("inputs must be on the GPU: this path has no CPU implementation")
        frames = vids[0].to(torch.float32).contiguous()
        valid = self._valid_region(samples, mask, frames)
        size = targets[0]["size"]
        img_h, img_w = float(size[0]), float(size[1])
        self._ensure_packed()
        ops.range_poll(frames.device)  # split-fp16 range guard: a tripped flag of an EARLIER forward raises here
        cached = self._text_lookup(ids, ids_host, frames.device)
        if cached is not None:  # text features of this expression are cached: the clip runs from them
            out = self.forward_features(frames, cached[0], cached[1], img_h, img_w, slot=slot, valid_hw=valid, select=select)
        else:  # one hipGraph per input shape: RoBERTa runs as a parallel branch beside the backbone, the decoder beside the pixel decoder
            ids = ids.to(frames.device)
            key = ("clip", tuple(frames.shape), tuple(ids.shape), img_h, img_w, self.training, int(slot), self._stamp, valid, select)
            out = self._dispatch(key, [frames], (ids,), self._group_text, img_h, img_w, (1, ids.shape[1]), slot,
                                 valid=valid, select=select)
        ops.range_snapshot_async(frames.device)
        return self._tag_diagnostics(out)

    # ---------------------------------------------------------------- eager launches, capture or replay: one place
    def _program(self, text_of, img_h, img_w, slot, kw):
        """run(frames, inputs, res=None): one pass of a launch program over the backbone's frame buffer `frames` and the non-frame
        inputs (live tensors or a capture's statics) -- eagerly on the slot's arena, or on a capture's resources `res`.  text_of
        maps the inputs to the `text` argument of _run, kw are _run's keywords (valid, groups, shared, select, index)."""
        def run(frames, inputs, res=None):
            return self._run(frames, text_of(*inputs), img_h, img_w, res, slot, **kw)
        return run

    @staticmethod
    def _like(frames, groups=1, shared=False, index=None, **_):
        """What _branch_resources sizes a capture by, from the backbone's frame buffer and _run's keywords: the frames the stages
        after the backbone see (a shared group: the one clip G times; an indexed group: G*Tc gathered frames, gather=True)."""
        rows = len(index) * len(index[0]) if index is not None else int(frames.shape[0]) * (groups if shared else 1)
        return types.SimpleNamespace(shape=(rows,) + tuple(frames.shape[1:]), device=frames.device, gather=index is not None)

    def _dispatch(self, key, sources, inputs, text_of, img_h, img_w, text_shape, slot=0, **kw):
        """The output dict of one launch program, from eager launches or from the replay of its captured graph (_want_graph).
        sources: the tensors whose rows, back to back, are the backbone's frame buffer (one clip, the clips of a group, the runs of
        a pool); inputs: the other input tensors; text_of, kw: see _program; text_shape = (captions, tokens each) of the text branch
        (_text_arena_extra).  A replay stages every source and input into the graph's statics with ONE copy launch: the sources go
        straight into their rows of the static frame buffer."""
        run = self._program(text_of, img_h, img_w, slot, kw)

        def frames_now():  # may alias the caller's tensor (one source) or be a fresh tensor (several)
            if len(sources) == 1:
                return sources[0].to(torch.float32).contiguous()
            return torch.cat([s.to(torch.float32) for s in sources], 0)

        if self._want_graph(key):
            ent = self._graphs.get(key)
            if ent is None:
                frames = frames_now().clone() if len(sources) == 1 else frames_now()
                st = [frames] + [t.clone() for t in inputs]
                ent = self._capture(key, st, lambda res: run(st[0], st[1:], res), self._like(frames, **kw), slot, text=text_shape)
            if ent is not None:
                buf, ends = ent.statics[0], accumulate(s.shape[0] for s in sources)
                # one source fills the buffer (no view to make on the per-clip path); several: their rows, back to back
                dsts = [buf] if len(sources) == 1 else [buf[e - s.shape[0]:e] for s, e in zip(sources, ends)]
                return self._replay(key, ent, dsts + ent.statics[1:], list(sources) + list(inputs))
            # the capture's arenas did not fit this shape's fallback kernels: eager from now on
        return run(frames_now(), inputs)

    def _pad_id(self):
        return int(getattr(getattr(self.text_encoder, "config", None), "pad_token_id", 1) or 1)

    def _check_caption_tokens(self, L):
        """ValueError for a caption of L tokens (the width of a [G, L] id tensor) beyond what the text encoder takes: part of the
        argument validation of every boundary, on the host and before any launch (text_encoder.max_caption_tokens)."""
        from .text_encoder import caption_too_long, max_caption_tokens
        emb = getattr(getattr(self.text_encoder, "embeddings", None), "position_embeddings", None)
        if emb is None:  # a text encoder that is not HuggingFace's RobertaModel: TextPlan refuses it on its own terms
            return
        limit = max_caption_tokens(emb.weight.shape[0], self._pad_id())
        if int(L) > limit:
            raise ValueError(caption_too_long(int(L), limit))

    def _group_text(self, ids, ragged=False):
        """The text callable of a launch program that starts from token ids (a clip or a clip group).  Ragged: the captions' lengths, key padding mask and position table
        come from the ids on the device in the same program (ops.caption_lens), so a captured graph follows the lengths that its
        static id buffer holds at each replay -- nothing about them is baked in at capture time."""
        if not ragged:
            return lambda alloc: self._text_plan().forward(ids, alloc)
        pad_id = self._pad_id()

        def text(alloc):
            rag = ops.caption_lens(ids, pad_id, alloc, self.cfg.hidden_dim)
            hid, pooled = self._text_plan().forward(ids, alloc, lens=rag[0])
            return hid, pooled, rag
        return text

    @torch.no_grad()
    def forward_group(self, clips, captions, targets, slot=0, ragged=False):
        """G independent clips in ONE launch program (an extension; `forward` is the reference's boundary).

        clips: list of G tensors [T,3,H,W] of the SAME shape on the GPU; captions: LongTensor [G, L] of token ids, or a list of G
        strings that tokenise to the same length; targets: [{'size': (H, W)}] (one entry, or G equal ones).  Returns a list of G
        output dicts, each what `forward([clip], caption, targets)` returns for that clip (same keys / shapes; values to fp32
        round-off: a launch with more rows may pick another split-K factor).  The clips do NOT interact -- the stages that look
        across a clip's frames or at its caption are block-diagonal per clip (pipeline._Clip) -- unlike the reference's own
        batch dimension, which mixes the clips of a batch.  Why: a clip alone leaves the GPU latency-bound for a third
        of its time (Swin stages 3-4 at 4600 rows, the text branch, the token / decoder paths); G clips share those launches:
        DESIGN section 3.10 has the measured clips/s.  Every position of `captions` [G, L] is a token: rows padded to a common
        length are INVALID input (rejected on the first sighting of a group shape).  Video-Swin's 3-D windows span a clip's frames: its window kernel is launched
        per clip, everything else is shared.  When `clips` holds the SAME tensor G times (G expressions of one video, the inner loop
        of inference_ytvos.py) the backbone runs once for the group.  Limits: one clip shape and one caption length per group, un-padded clips, G <= 64 (the
        text layers leave the weight-stream kernels for the tiled GEMMs above 128 caption tokens in all).

        ragged=True (opt-in): the captions may have different token lengths.  Strings are tokenised as `forward` tokenises them
        and right-padded with the pad id to the longest; a LongTensor [G, Lmax] is taken as right-padded with pad_token_id
        (caption g's length = index of its first pad id, Lmax if none, at least 1; derived on the device, no read-back).  Host ids
        with an interior pad or an empty caption raise ValueError.  Each clip's result is its B = 1 forward on the un-padded
        caption: the text self-attention and every text cross-attention take the pads as masked keys, the 1-D position map is
        normalised by each caption's length (position_encoding.py:28-50).  One captured graph serves every length mix of a
        (G, Lmax, clip shape).

        Single-frame groups (A2D-Sentences / JHMDB-Sentences: one annotated frame per clip, tce_rvos.py:233-243): EVERY target
        carries 'valid_indices' (an int or a 1-element tensor, as the datasets give it; `targets` then holds G entries).  The
        backbone sees all G*Tc frames (Video-Swin's windows stay per clip), after every stage the rows of frame valid_indices[g] of
        clip g are gathered into a dense map (pipeline.pick_segments, tce_copy_segments) and the rest is the group program with one
        frame per clip.  Each result is what forward([clip], caption, [{'size', 'valid_indices'}]) returns.  The indices are read on
        the host (device tensors: one read-back) and the index tuple is part of the graph key: the gather's source addresses are
        baked into the copy launches' arguments, so every distinct tuple of a shape captures a graph of its own (the LRU bound on
        the graph cache, max_graphs / max_graph_bytes, limits what that costs; callers bucket by index -- video.plan_single_frame_groups).
        A shared group (the same tensor G times) runs the backbone once; the indices may differ per caption.  Targets of which some
        carry 'valid_indices' and others do not raise ValueError, an index outside the clip IndexError."""
        G = len(clips)
        ids, single = self._group_captions(captions, G, ragged, clips[0].device, "clip groups")
        if single is not None:
            return [self.forward([clips[0]], single, targets[:1], slot=slot)]
        shp = tuple(clips[0].shape)
        if any(tuple(c.shape) != shp or not c.is_cuda for c in clips) or len(shp) != 4:
            raise ValueError("clip groups: G CUDA tensors [T,3,H,W] of one shape")
        if ids.dim() != 2 or ids.shape[0] != G or G > 64:
            raise ValueError("clip groups: token ids [G, L], G <= 64")
        img_h, img_w = self._group_size(targets, "clip groups")
        sel = self._group_select(targets, G, shp[0])
        self._ensure_packed()
        ops.range_poll(clips[0].device)
        ids = ids.to(clips[0].device)
        # one clip, G captions (the expressions of a video: the SAME tensor G times): the backbone runs once
        shared = all(c is clips[0] for c in clips[1:])
        if ragged:
            ids = ids.to(torch.int64).contiguous()
        # ragged: the flag, never the lengths (they live in the static id buffer)
        key = ("group", G, shared, shp, tuple(ids.shape), img_h, img_w, self.training, int(slot), self._stamp) + (("ragged",) if ragged else ())
        if sel is not None:  # the selection's source addresses are arguments of the captured copy launches: one graph per index tuple
            key += (("select", sel),)
        if not ragged:
            self._refuse_pad_ids(key, ids, "clip groups", "padded captions are not supported -- group captions of equal token "
                                                          "length (every position of [G, L] is taken as a token)")
        out = self._dispatch(key, clips[:1] if shared else list(clips), (ids,), lambda i: self._group_text(i, ragged), img_h, img_w,
                             (G, ids.shape[1]), slot, groups=G, shared=shared, select=sel)
        ops.range_snapshot_async(clips[0].device)
        return self._split_group(out, G, shp[0] if sel is None else 1)

    def _group_captions(self, captions, G, ragged, device, what, one_length_hint=""):
        """The captions of a group boundary (`what` names it in the messages), normalised on the host and before any launch:
        (token ids [G, L], None) -- or, for G = 1, (None, the caption to hand to `forward`).  Strings are tokenised as `forward`
        tokenises them.  A caption beyond the text encoder's limit is refused first.  ragged: strings are right-padded with the
        pad id to the longest, host ids are validated as right-padded (caption_lengths); not ragged: strings must tokenise to one
        length."""
        rows = None
        if isinstance(captions, (list, tuple)):
            rows = [self._tokenise([c], device)[0] for c in captions]
            self._check_caption_tokens(max(int(r.shape[1]) for r in rows))
        elif captions.dim() == 2:
            self._check_caption_tokens(captions.shape[1])
        if ragged:
            if rows is not None:
                captions, _ = pad_captions(rows, self._pad_id())
            elif not captions.is_cuda:
                caption_lengths(captions, self._pad_id())  # validation only: the device derives the lengths itself
        if G == 1:
            cap = captions[:1] if torch.is_tensor(captions) else [captions[0]]
            if ragged and torch.is_tensor(cap):  # one caption: no padding needed (its length on the host: one read-back)
                cap = cap[:, :caption_lengths(cap.cpu(), self._pad_id())[0]]
            return None, cap
        if torch.is_tensor(captions):
            return captions, None
        if len({int(r.shape[1]) for r in rows}) != 1:
            raise ValueError(f"{what}: the captions must tokenise to one length{one_length_hint}")
        return torch.cat(rows, 0), None

    @staticmethod
    def _group_size(targets, what):
        """(img_h, img_w) of a group's targets: one entry, or G equal ones."""
        size = targets[0]["size"]
        img_h, img_w = float(size[0]), float(size[1])
        if any((float(t["size"][0]), float(t["size"][1])) != (img_h, img_w) for t in targets[1:]):
            raise ValueError(f"{what}: the clips of a group share one target size")
        return img_h, img_w

    def _refuse_pad_ids(self, key, ids, what, advice):
        """A [G, L] id tensor built by PADDING G captions to one length would silently differ from each clip's B = 1 forward in a
        group that is not ragged (the text kernels take every position as a token; the reference masks pads through attention_mask
        / key_padding_mask): checked ONCE per group shape `key`, on its first sighting (a device read-back)."""
        if key not in self._group_checked:
            self._group_checked.add(key)
            pad_id = self._pad_id()
            if bool((ids == pad_id).any()):
                raise ValueError(f"{what}: token ids contain the pad id ({pad_id}): {advice}")

    def _pool_plan(self, index, F):
        """(index as a tuple of G int tuples, the pool frames the backbone runs over in its row order) of an indexed group over a
        pool of F frames (pipeline.pool_segments: distinct frames for the 2-D backbones, distinct clips for Video-Swin)."""
        from .pipeline import pool_segments
        idx = tuple(tuple(int(v) for v in t) for t in index)
        if not idx or not idx[0] or any(len(t) != len(idx[0]) for t in idx):
            raise ValueError("indexed groups: G >= 1 index tuples of one length Tc >= 1")
        if len(idx) > 64:
            raise ValueError("indexed groups: G <= 64")
        if any(not 0 <= v < F for t in idx for v in t):
            raise ValueError(f"indexed groups: an index lies outside the pool's {F} frames")
        return idx, pool_segments(idx, [(1, 1)], [1], "clip" if self.cfg.video else "frame")[0]

    @torch.no_grad()
    def forward_indexed(self, pool, index, captions, targets, ragged=False, slot=0):
        """A clip group whose clips are index tuples into a pool of frames (an extension, like forward_group): one backbone pass per
        DISTINCT frame, whatever number of (clip, caption) slots read it -- the windows of a video that overlap by their context
        frames, each under several captions (video.run_video_windows(share="frames")).

        pool: [F,3,H,W] un-padded frames on the GPU; index: G tuples of Tc ints in [0, F), clip g = pool[list(index[g])] -- a frame may
        serve several clips and several positions of one clip; captions (one per slot; a caption may repeat), targets, ragged, slot
        as in forward_group.  Returns G output dicts: result g is what forward([pool[list(index[g])]], captions[g], targets) returns
        (same keys / shapes, values to the round-off forward_group documents).

        The 2-D backbones (swin_*, resnet*) are frame-independent: the backbone runs over the distinct frames of `index`, U rows in
        increasing pool order.  Video-Swin's 3-D windows span a clip, so its unit is the clip: the backbone runs over the distinct
        index tuples in order of first appearance, one window launch per distinct clip.  After every backbone stage the rows of each
        slot's frames are gathered into the dense map of the group program (pipeline.pool_segments, tce_copy_segments, issued where
        the map's consumer runs); an identity gather launches nothing.  The text stage sees G captions: repeated captions are not
        de-duplicated.  The gather's source addresses are arguments of the captured copy launches, so the index tuple is part of the
        graph key (as valid_indices is): callers that want few graphs keep their indices relative to the pool.  G = 1 goes to
        `forward`.  ValueError: 'valid_indices' in a target, an index outside the pool, tuples of different lengths, G > 64,
        G != len(captions); NotImplementedError: padded input (a NestedTensor)."""
        if hasattr(pool, "tensors") and hasattr(pool, "mask"):
            raise NotImplementedError("indexed groups: un-padded frames only (a [F,3,H,W] tensor, not a NestedTensor)")
        if not torch.is_tensor(pool) or pool.dim() != 4 or pool.shape[1] != 3:
            raise ValueError("indexed groups: the pool is one tensor [F,3,H,W]")
        if any("valid_indices" in t for t in targets):
            raise ValueError("indexed groups: 'valid_indices' is not supported over a pool")
        index, need = self._pool_plan(index, int(pool.shape[0]))
        G, Tc = len(index), len(index[0])
        if (len(captions) if isinstance(captions, (list, tuple)) else int(captions.shape[0])) != G:
            raise ValueError(f"indexed groups: {G} index tuples but "
                             f"{len(captions) if isinstance(captions, (list, tuple)) else int(captions.shape[0])} captions")
        dev = pool.device
        ids, single = self._group_captions(captions, G, ragged, dev, "indexed groups", " (or ragged=True)")
        if not pool.is_cuda:
            raise RuntimeError("inputs must be on the GPU: this path has no CPU implementation")
        if single is not None:
            return [self.forward([pool[list(index[0])]], single, targets[:1], slot=slot)]
        if ids.dim() != 2:
            raise ValueError("indexed groups: token ids [G, L]")
        img_h, img_w = self._group_size(targets, "indexed groups")
        self._ensure_packed()
        ops.range_poll(dev)
        ids = ids.to(dev)
        if ragged:
            ids = ids.to(torch.int64).contiguous()
        key = ("indexed", G, tuple(pool.shape), tuple(ids.shape), img_h, img_w, self.training, int(slot), self._stamp) + \
            (("ragged",) if ragged else ()) + (("index", index),)
        # the backbone's frames as runs of consecutive pool frames: [first pool frame, frames]
        runs = []
        for f in need:
            if runs and runs[-1][0] + runs[-1][1] == f:
                runs[-1][1] += 1
            else:
                runs.append([f, 1])
        if not ragged:  # once per group shape, whatever the index
            self._refuse_pad_ids(key[:-1], ids, "indexed groups", "padded captions need ragged=True")
        out = self._dispatch(key, [pool[a:a + n] for a, n in runs], (ids,), lambda i: self._group_text(i, ragged), img_h, img_w,
                             (G, ids.shape[1]), slot, groups=G, index=index)
        ops.range_snapshot_async(dev)
        return self._split_group(out, G, Tc)

    def _split_group(self, out, G, Tc):
        """The output dict of a whole group -> one dict per clip (Tc output frames each)."""
        def part(v, g):  # clip g's slice of an output of the whole group
            if v.dim() >= 2 and v.shape[0] == 1 and v.shape[1] == G * Tc:
                return v[:, g * Tc:(g + 1) * Tc]
            return v[g * Tc:(g + 1) * Tc]  # memory [G*Tc, S, 256]

        outs = []
        for g in range(G):
            o = {}
            for k, v in out.items():
                if torch.is_tensor(v):
                    o[k] = part(v, g)
                elif k == "aux_outputs":
                    o[k] = [{kk: part(vv, g) for kk, vv in a.items()} for a in v]
            outs.append(self._tag_diagnostics(o))
        return outs

    @staticmethod
    def _group_select(targets, G, Tc):
        """The per-clip annotated-frame indices of a group's targets as a tuple of G ints, or None when no target carries
        'valid_indices'.  Read on the host; device tensors cost ONE read-back for the group."""
        has = ["valid_indices" in t for t in targets]
        if not any(has):
            return None
        if not all(has) or len(targets) != G:
            raise ValueError("clip groups: the single-frame path needs 'valid_indices' in every one of the G targets")
        vals = [t["valid_indices"] for t in targets]
        if any(torch.is_tensor(v) and v.numel() != 1 for v in vals):
            raise ValueError("clip groups: valid_indices is one index per clip (an int or a 1-element tensor)")
        if any(torch.is_tensor(v) and v.is_cuda for v in vals):
            dev = next(v.device for v in vals if torch.is_tensor(v) and v.is_cuda)
            vals = torch.stack([torch.as_tensor(v).reshape(()).to(dev, torch.int64) for v in vals]).tolist()
        sel = tuple(int(v) for v in vals)
        for v in sel:
            if not 0 <= v < Tc:
                raise IndexError(f"valid_indices {v} outside the clip's {Tc} frames")
        return sel

    @staticmethod
    def _tag_diagnostics(out):
        """A diagnostic launch program (TCE_ABLATE: stages skipped) marks every result it returns as garbage."""
        from . import pipeline
        if pipeline.ABLATE:
            out["ablated"] = sorted(pipeline.ABLATE)
        return out

    @staticmethod
    def _valid_region(samples, mask, frames):
        """(rows, columns) of the clip's frames that are NOT padding, or None for an un-padded clip.  Padding = a rectangular
        border at the bottom / right, the same in every frame (what nested_tensor_from_videos_list produces, util/misc.py:
        354-377); any other mask is rejected.  Host metadata when the NestedTensor carries it, else ONE device read-back."""
        if mask is None or getattr(samples, "unpadded", False):
            return None
        H, W = int(frames.shape[-2]), int(frames.shape[-1])
        vhw = getattr(samples, "valid_hw", None)
        if vhw is not None:
            hv, wv = vhw[0]
        else:
            m = mask[0]
            hv, wv = int((~m[0, :, 0]).sum()), int((~m[0, 0, :]).sum())
            rect = torch.ones(H, W, dtype=torch.bool, device=m.device)
            rect[:hv, :wv] = False
            if hv < 1 or wv < 1 or not bool((m == rect[None]).all()):
                raise NotImplementedError("padding masks other than a bottom / right border shared by all frames are not supported")
        return None if (hv, wv) == (H, W) else (int(hv), int(wv))

    def _want_graph(self, key):
        """Graph replay for shapes that come back; eager launches for the first `graph_after` sightings of a shape."""
        if not self.use_graph or key in self._nograph:
            return False
        if key in self._graphs:
            return True
        n = self._sightings.get(key, 0)
        self._sightings[key] = n + 1
        self._sightings.move_to_end(key)
        while len(self._sightings) > 256:
            self._sightings.popitem(last=False)
        if n < self.graph_after:
            return False
        if len(_ALL_GRAPHS) >= GRAPH_BUDGET and not (GRAPH_OWN_EXEC and not KEEP_GRAPHS):
            global _BUDGET_WARNED
            if not _BUDGET_WARNED:
                _BUDGET_WARNED = True
                import warnings
                warnings.warn(f"tce_rvos_amd: the process's hipGraph capture budget ({GRAPH_BUDGET}, TCE_GRAPH_BUDGET) is spent: "
                              f"shapes that are not cached now run as eager launches (same results, ~15 % slower per clip); "
                              f"model.graph_state() reports this", RuntimeWarning, stacklevel=3)
            return False
        return True

    @staticmethod
    def graph_state():
        return graph_state()

    # ---------------------------------------------------------------- per-expression text cache
    def _text_lookup(self, ids, ids_host=None, device=None):
        """(last_hidden_state [L,768], pooler_output [768]) of a cached expression or None.  The reference recomputes
        RoBERTa for every clip of an expression (tce_rvos.py:406-424 inside forward; inference_ytvos.py:184-230 loops
        the clips); with `text_cache_size > 0` the features are computed once per distinct token sequence.  The
        lookup key is the token ids on the HOST, so the cache is meant for string captions / host id tensors."""
        if self.text_cache_size <= 0:
            return None
        key = tuple(int(v) for v in (ids if ids_host is None else ids_host).reshape(-1).tolist())  # device ids: one sync
        ent = self._text_cache.get(key)
        if ent is None:
            ids = ids.to(device) if device is not None else ids
            hid, pooled = self._text_plan().forward(
                ids, lambda *shape: torch.empty(*shape, dtype=torch.float32, device=ids.device))
            ent = (hid, pooled)
            self._text_cache[key] = ent
            while len(self._text_cache) > self.text_cache_size:
                self._text_cache.popitem(last=False)
        else:
            self._text_cache.move_to_end(key)
        return ent

    def _tokenise(self, captions, device):
        if isinstance(captions, (list, tuple)):
            if isinstance(self.tokenizer, SyntheticTokenizer):
                ids, att = self.tokenizer(list(captions))  # host tensors
            else:  # a HuggingFace tokenizer, called as the reference calls it (tce_rvos.py:408)
                tok = self.tokenizer.batch_encode_plus(list(captions), padding="longest", return_tensors="pt")
                ids, att = tok["input_ids"], tok["attention_mask"]
            if bool((att != 1).any()):
                raise NotImplementedError("padded captions (B > 1) are not supported")
        else:  # token ids: every position is a token (no device read-back here: it would serialise consecutive clips)
            ids, att = captions, None
        # host ids stay on the host until something needs them on the device (a cache hit never does: an H2D copy of pageable
        # memory per clip would wait for the stream and stop the host from running ahead of the GPU)
        return ids, att, (None if ids.is_cuda else ids)

    def _text_plan(self):
        """RoBERTa on the HIP kernels (text_encoder.py); the HF module only owns the weights."""
        if self._text is None:
            from .text_encoder import TextPlan
            self._text = TextPlan(self.text_encoder)
        return self._text

    def text_encoder_reference(self, ids, att=None):
        """HuggingFace's own forward of the same module -- the CHECKER of the HIP text path (tests only)."""
        att = torch.ones_like(ids) if att is None else att
        enc = self.text_encoder(input_ids=ids, attention_mask=att)
        return enc.last_hidden_state.float(), enc.pooler_output.float()

    def _run(self, frames, text, img_h, img_w, res, slot=0, valid=None, groups=1, shared=False, select=None, index=None):
        from .pipeline import run_clip
        T, _, H0, W0 = frames.shape
        if res is None:  # eager: the slot's arena, single stream
            if index is not None:  # the group's G*Tc frames, and the gathered maps beside the backbone's
                rows = len(index) * len(index[0])
                ar = self._get_arena(rows, H0, W0, frames.device, slot, extra=sum(self._gather_bytes(rows, H0, W0)))
            else:
                ar = self._get_arena(T * (groups if shared else 1), H0, W0, frames.device, slot)
            return run_clip(self, frames, text, img_h, img_w, ar, valid=valid, groups=groups, shared=shared, select=select, index=index)
        return run_clip(self, frames, text, img_h, img_w, res.arena, res.side_arena, res.side_stream, clone_outputs=False, valid=valid,
                        groups=groups, shared=shared, select=select, index=index,
                        fork2=(res.arena2, res.stream2) if FORK2 else None,
                        fork3=((res.arena3, res.stream3), (res.arena4, res.stream4)) if FORK3 else None)

    def _text_arena_extra(self, text):
        """Bytes the text branch of text = (G captions, L tokens each) needs in its arena beyond the flat allowance of
        _branch_resources, which was sized for captions of up to 128 tokens: 0 up to there (those shapes keep the arenas they had).
        Per token row: RoBERTa's activations (x, packed qkv, attention output, the MLP's hidden row and one GEMM workspace row of
        that width) and the 256-wide rows after the resizer (its two maps, keys and values of the five cross-attention sites, a
        ragged group's position table), rounded up."""
        if text is None or int(text[1]) <= 128:
            return 0
        tc = getattr(self.text_encoder, "config", None)
        C, ff = int(getattr(tc, "hidden_size", 768)), int(getattr(tc, "intermediate_size", 3072))
        return int(text[0]) * int(text[1]) * 4 * (5 * C + ff + max(ff, 3 * C) + 16 * self.cfg.hidden_dim) + (8 << 20)

    def _branch_resources(self, like, slot=0, text=None):
        """The _Resources of one capture, sized by `like` (_like): the main arena
        and one arena per parallel branch that allocates; the side streams are the (device, slot)'s shared set.  like.gather (an
        indexed group): T frames' maps are gathered from the backbone's -- room for each in the arena of the branch that consumes it
        (stage 0: the stride-4 lateral branch, stages 1 / 2: the early input projections) and for all of them in the main arena."""
        T, _, H0, W0 = like.shape
        tok0 = T * ((H0 + 3) // 4) * ((W0 + 3) // 4)
        st = _side_streams(like.device, slot)
        gb = self._gather_bytes(T, H0, W0) if getattr(like, "gather", False) else [0, 0, 0, 0]
        return _Resources(  # constructed in field order
                ops.Arena(like.device, self._arena_bytes(T, H0, W0) + sum(gb)),
                ops.Arena(like.device, T * self._tokens_per_frame(H0, W0) * 256 * 4 * 4 + (32 << 20) + self._text_arena_extra(text)),
                st[0],
                # third branch: the pixel decoder's stride-4 lateral path (tgt + its self-attention / FFN temporaries)
                ops.Arena(like.device, int(tok0 * 4 * (2048 * 1.1 + 256 * 4)) + (64 << 20) + gb[0]),
                st[1],
                # fourth / fifth branch: the stride-32 lateral path + the merge chain down to stride 16 (tokens/64 and
                # tokens/16 maps, two-GEMM FFN hidden [tokens/16 ... , 2048]); the stride-16 lateral path.  With the early
                # input projections the fourth also hosts encoder level 0 (tokens/4 rows): sized for its UNFUSED form
                # (projection, GroupNorm output, q, attention output + workspaces: 5 maps of [tokens/4, 256]) -- the form
                # exact-fp32 mode and captions longer than 32 tokens take
                ops.Arena(like.device, max(int(tok0 / 64 * 4 * (2048 + 256 * 12)) + int(tok0 / 16 * 4 * 256 * 8),
                                           int(tok0 / 4 * 4 * 256 * 5)) + (64 << 20) + self._conv3_ws_bytes(T, H0, W0, (16, 32)) + gb[1]),
                st[2],
                ops.Arena(like.device, int(tok0 / 16 * 4 * (2048 * 1.1 + 256 * 12)) + (64 << 20) + gb[2]),
                st[3])

    @torch.no_grad()
    def hazard_check(self, frames, ids, img_hw=None, valid=None, slot=0, dry=False, groups=1, shared=False, ragged=False, observe=None,
                     select=None, index=None):
        """Records ONE pass of the clip's launch program on the capture topology (the same arenas, side streams, forks and
        joins a captured graph is built from) and checks it for races: any two launches not ordered by a fork / join edge
        must touch disjoint memory (tce_rvos_amd/hazard.py).  frames [T,3,H,W] and token ids [1,L] on the GPU.
        dry=True: the recorded pass launches nothing (negative controls).  ragged=True: the ragged clip-group program
        (forward_group(..., ragged=True); ids [groups, Lmax] right-padded).  select: the single-frame path -- one index (groups = 1)
        or one per clip of the group (with groups= / shared=: forward_group's valid_indices program).  index: forward_indexed's
        program -- `frames` is then the pool [F,3,H,W], `index` the group's tuples of pool indices and ids [len(index), L] (groups is
        taken from it).  Returns a hazard.Report (`.clean`, `str()`);
        results of the pass are discarded.  observe (tests): called as observe("before", resources, None) after the warm-up pass
        and observe("after", resources, recorder) after the recorded one, everything synchronised; it only looks on."""
        from . import hazard
        frames = frames.to(torch.float32).contiguous()
        if index is not None:  # an indexed group: `frames` is the pool, the program runs on the frames its backbone needs
            index, need = self._pool_plan(index, int(frames.shape[0]))
            groups = len(index)
            frames = frames[need].contiguous()
        T, _, H0, W0 = frames.shape
        img_h, img_w = (float(H0), float(W0)) if img_hw is None else (float(img_hw[0]), float(img_hw[1]))
        self._ensure_packed()
        if select is not None:
            select = int(select) if groups == 1 and not isinstance(select, (tuple, list)) else tuple(int(v) for v in select)
        kw = dict(valid=valid, groups=groups, shared=shared, select=select, index=index)
        res = self._branch_resources(self._like(frames, **kw), slot, text=(groups, ids.shape[1]))
        st = (frames.clone(), ids.to(frames.device).clone())
        program = self._program(lambda i: self._group_text(i, ragged), img_h, img_w, slot, kw)
        run = lambda: program(st[0], st[1:], res)  # noqa: E731
        main = torch.cuda.Stream(device=frames.device)  # like a capture: never the legacy default stream (it syncs with all)
        main.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(main):
            if not dry:  # warm-up: per-shape constants and lazy initialisations (host syncs) happen here, not in the record
                run()
            torch.cuda.synchronize()
            if observe is not None:
                observe("before", res, None)
                torch.cuda.synchronize()
            sd = self._text_plan().sd  # rows of these are gathered by token id: the models need their extents
            with hazard.recording(dry=dry, tables=[sd["embeddings.word_embeddings.weight"], sd["embeddings.position_embeddings.weight"]]) as rec:
                run()
            torch.cuda.synchronize()
            if observe is not None:
                observe("after", res, rec)
        torch.cuda.current_stream().wait_stream(main)
        return rec.analyse()

    def _capture(self, key, statics, fn, like, slot=0, text=None):
        """Captures fn((arena, side_arena, side_stream, ...)) into a graph; the arenas belong to the graph (their
        addresses are baked into it), the side streams are the (device, slot)'s shared set.  Returns None (and pins the
        key to the eager path) if a branch arena turns out too small for this shape's kernels.  text: (captions, tokens each) of
        the program's text branch (_text_arena_extra)."""
        res = self._branch_resources(like, slot, text=text)
        try:
            fn(res)  # eager warm-up on the same resources: builds per-shape constants, lazy inits
        except MemoryError as e:
            import warnings
            torch.cuda.synchronize()
            self._nograph.add(key)
            warnings.warn(f"tce_rvos_amd: graph capture of {key[:2]} skipped ({e}); this shape runs eagerly", RuntimeWarning)
            return None
        torch.cuda.synchronize()
        own = GRAPH_OWN_EXEC and not KEEP_GRAPHS
        graph = torch.cuda.CUDAGraph(keep_graph=True) if (KEEP_GRAPHS or own) else torch.cuda.CUDAGraph()
        # capture_error_mode="thread_local": under the default ("global") mode ANY thread's event query is an error while this
        # thread captures -- and torch.distributed's RCCL watchdog thread polls the events of in-flight collectives (bench.py keeps
        # the previous step's all-gather in flight): it then dies with "operation not permitted when stream is capturing" and takes
        # the process down (seen once in round 4, test_rccl_world1_bench_path_executes_the_collective).  This thread itself calls
        # nothing capture-unsafe: arenas and side streams exist before the capture starts.
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = fn(res)
        if own:
            import ctypes as C
            from ._lib import lib
            raw = (C.c_void_p * 1)(int(graph.raw_cuda_graph()))
            ex = C.c_void_p()
            if lib().tce_graph_group(raw, 1, C.byref(ex)) == 0 and ex.value:
                del graph  # the captured hipGraph_t was never instantiated: nothing else refers to it
                graph = _OwnedExec(ex)
            else:  # a node kind the re-creation does not know (none in the shipped program): the legacy, never-destroyed path
                own = False
                graph.instantiate()
        elif KEEP_GRAPHS:
            graph.instantiate()
        if not own:
            _ALL_GRAPHS.append(graph)  # legacy executables outlive their cache entry (see _ALL_GRAPHS)
        try:
            plan = ops.CopyPlan(_flat_outputs(out)) if COPYPLAN else None
        except ValueError:  # an output the segment copy cannot express: per-tensor clones
            plan = None
        ent = _Entry(graph, statics, out, res, sum(r.buf.numel() for r in res if isinstance(r, ops.Arena)), plan)
        self._graphs[key] = ent
        # LRU bound (entries and bytes); the entry just captured always stays.  Eviction returns the arenas.
        while len(self._graphs) > 1 and (len(self._graphs) > self.max_graphs or
                                         sum(e.nbytes for e in self._graphs.values()) > self.max_graph_bytes):
            torch.cuda.synchronize()  # the evicted graph may still be replaying
            _, old = self._graphs.popitem(last=False)
            if isinstance(old.exe, _OwnedExec):
                old.exe.destroy()  # owned executables go with their entry (legacy ones stay in _ALL_GRAPHS)
        return ent

    @staticmethod
    def _tokens_per_frame(H0, W0):
        h, w = (H0 + 3) // 4, (W0 + 3) // 4
        n = 0
        for _ in range(3):
            h, w = (h + 1) // 2, (w + 1) // 2
            n += h * w
        return n + ((h + 1) // 2) * ((w + 1) // 2)

    def _replay(self, key, ent, dsts, srcs):
        """dsts: views of ent.statics, one per tensor of srcs."""
        self._graphs.move_to_end(key)
        ops.copy_many(dsts, srcs)  # one launch stages the inputs ...
        ent.exe.replay()
        if ent.plan is None:
            return {k: (v.clone() if torch.is_tensor(v) else [{kk: vv.clone() for kk, vv in a.items()} for a in v])
                    for k, v in ent.out.items()}
        it = iter(ent.plan.clone())  # ... and one hands back fresh output tensors (same order as _flat_outputs)
        return {k: (next(it) if torch.is_tensor(v) else [{kk: next(it) for kk in a} for a in v]) for k, v in ent.out.items()}

    @torch.no_grad()
    def forward_text_encoder(self, captions, device):
        """tce_rvos.py:406-424 up to the RoBERTa outputs: (last_hidden_state [1,L,768], pooler_output [1,768])."""
        ids, att, _ = self._tokenise(captions, device)
        ids = ids.to(device)
        hid, pooled = self._text_plan().forward(
            ids, lambda *shape: torch.empty(*shape, dtype=torch.float32, device=ids.device))
        return hid[None], pooled[None]

    @torch.no_grad()
    def forward_features(self, frames, text_hidden, text_pooled, img_h, img_w, slot=0, valid_hw=None, select=None, groups=1,
                         shared=False):
        """Everything after the text encoder.  frames [T,3,H,W]; text_hidden [L,768]; text_pooled [768].  valid_hw = (rows,
        columns) of the frames that are not padding (a clip zero-padded at the bottom / right; None: un-padded).  select: the
        annotated frame of the single-frame path (targets[0]['valid_indices'], tce_rvos.py:233-243; None: every frame).
        groups = G > 1: a clip group from given text features (forward_group's program): frames [G*Tc,3,H,W] (the clips back to
        back; shared=True: ONE clip's [Tc,3,H,W]), text_hidden [G*L,768] caption-major, text_pooled [G,768], select None or a
        sequence of G indices (one per clip); un-padded clips only.  Returns a list of G output dicts."""
        if int(groups) > 1:
            return self._forward_features_group(frames, text_hidden, text_pooled, img_h, img_w, slot, valid_hw, select, int(groups),
                                                bool(shared))
        if valid_hw is not None:
            valid_hw = (int(valid_hw[0]), int(valid_hw[1]))
            if valid_hw == (int(frames.shape[-2]), int(frames.shape[-1])):
                valid_hw = None
        self._ensure_packed()
        text_hidden, text_pooled = text_hidden.contiguous(), text_pooled.contiguous()
        select = None if select is None else int(select)
        key = ("feat", tuple(frames.shape), int(text_hidden.shape[0]), float(img_h), float(img_w), self.training, int(slot),
               self._stamp, valid_hw, select)
        return self._tag_diagnostics(self._dispatch(key, [frames], (text_hidden, text_pooled), lambda hid, pooled: (hid, pooled),
                                                    img_h, img_w, (1, text_hidden.shape[0]), slot, valid=valid_hw, select=select))

    def _forward_features_group(self, frames, text_hidden, text_pooled, img_h, img_w, slot, valid_hw, select, G, shared):
        if valid_hw is not None and (int(valid_hw[0]), int(valid_hw[1])) != (int(frames.shape[-2]), int(frames.shape[-1])):
            raise NotImplementedError("clip groups: un-padded clips only")
        Tb = int(frames.shape[0])
        if frames.dim() != 4 or (not shared and Tb % G) or text_hidden.dim() != 2 or text_hidden.shape[0] % G or \
                tuple(text_pooled.shape) != (G, text_hidden.shape[1]) or G > 64:
            raise ValueError("clip groups from text features: frames [G*Tc,3,H,W] (shared: [Tc,3,H,W]), text_hidden [G*L,768], "
                             "text_pooled [G,768], G <= 64")
        Tc = Tb if shared else Tb // G
        sel = None
        if select is not None:
            sel = tuple(int(v) for v in (select.tolist() if torch.is_tensor(select) else select))
            if len(sel) != G:
                raise ValueError(f"clip groups: {G} clips but {len(sel)} selected frames")
            for v in sel:
                if not 0 <= v < Tc:
                    raise IndexError(f"valid_indices {v} outside the clip's {Tc} frames")
        self._ensure_packed()
        frames = frames.to(torch.float32).contiguous()
        text_hidden, text_pooled = text_hidden.contiguous(), text_pooled.contiguous()
        key = ("featgroup", G, shared, tuple(frames.shape), int(text_hidden.shape[0]), float(img_h), float(img_w), self.training,
               int(slot), self._stamp, sel)
        out = self._dispatch(key, [frames], (text_hidden, text_pooled), lambda hid, pooled: (hid, pooled), img_h, img_w,
                             (G, text_hidden.shape[0] // G), slot, groups=G, shared=shared, select=sel)
        return self._split_group(out, G, Tc if sel is None else 1)


def caption_lengths(ids, pad_id):
    """Token counts of right-padded host ids [G, Lmax] (ragged clip groups): caption g's length is the index of its first pad id,
    Lmax if it has none.  ValueError for a caption with no token or a pad id followed by a non-pad id."""
    if not torch.is_tensor(ids) or ids.dim() != 2:
        raise ValueError("ragged captions: token ids [G, Lmax]")
    lens = []
    for g, row in enumerate(ids.tolist()):
        n = row.index(pad_id) if pad_id in row else len(row)
        if n == 0:
            raise ValueError(f"ragged captions: caption {g} has no token")
        if any(t != pad_id for t in row[n:]):
            raise ValueError(f"ragged captions: caption {g} has a pad id inside it (position {n}): pads go at the right end only")
        lens.append(n)
    return lens


def pad_captions(rows, pad_id):
    """Host id rows [1, L_g] of G captions -> (ids [G, Lmax] right-padded with pad_id, lengths).  Validated as caption_lengths."""
    rows = [r.reshape(-1).to(torch.int64).cpu() for r in rows]
    if not rows:
        raise ValueError("ragged captions: no caption")
    Lmax = max(int(r.numel()) for r in rows)
    ids = torch.full((len(rows), Lmax), int(pad_id), dtype=torch.int64)
    for g, r in enumerate(rows):
        ids[g, :r.numel()] = r
    lens = caption_lengths(ids, pad_id)
    if lens != [int(r.numel()) for r in rows]:
        raise ValueError("ragged captions: a caption contains the pad id")
    return ids, lens


def _flat_outputs(out):
    """The tensors of forward()'s output dict in iteration order (aux_outputs: list of dicts)."""
    flat = []
    for v in out.values():
        if torch.is_tensor(v):
            flat.append(v)
        else:
            for a in v:
                flat.extend(a.values())
    return flat


def is_frozen_bn_key(key):
    from .weights import _FBN
    return _FBN.search(key) is not None


def v_is_conv(t):
    return t.dim() == 4


def build_text_encoder(args=None):
    """RoBERTa-base architecture from the installed `transformers` package.  The reference fetches
    'roberta-base' by name (tce_rvos.py:136-137): no network here, so weights come from a local directory when
    `args.text_encoder_path` is given, else random initialisation under a fixed seed."""
    import transformers
    path = getattr(args, "text_encoder_path", None) if args is not None else None
    if path:
        return transformers.RobertaModel.from_pretrained(path)
    layers = getattr(args, "text_encoder_layers", 12) if args is not None else 12
    cfg = transformers.RobertaConfig(vocab_size=50265, max_position_embeddings=514, type_vocab_size=1, pad_token_id=1,
                                     num_hidden_layers=layers)
    st = torch.random.get_rng_state()
    torch.manual_seed(0)
    m = transformers.RobertaModel(cfg)
    torch.random.set_rng_state(st)
    return m.eval()


def build_tokenizer(args=None):
    """The reference builds RobertaTokenizerFast.from_pretrained('roberta-base') (tce_rvos.py:136, a download).  With
    `args.text_encoder_path` (a local copy of the checkpoint) the real tokenizer is loaded from the same directory --
    real weights with hashed ids would give wrong masks silently, so a failure to load it is an error.  Without a
    path the text weights are random anyway and a deterministic hashing stand-in keeps string captions usable."""
    path = getattr(args, "text_encoder_path", None) if args is not None else None
    if not path:
        return SyntheticTokenizer()
    import transformers
    try:
        return transformers.RobertaTokenizerFast.from_pretrained(path)
    except Exception as e:  # noqa: BLE001
        raise RuntimeError(f"text_encoder_path={path!r}: the RoBERTa weights load from there but the tokenizer files "
                           f"(vocab.json / merges.txt / tokenizer.json) do not ({e}); pass tokenizer=... explicitly or "
                           f"call the model with token ids") from e


class _Stub(nn.Module):
    """Stands where the reference returns a piece that is out of scope (the post-processor tests use it)."""

    def __init__(self, what):
        super().__init__()
        self.what = what

    def forward(self, *a, **k):
        raise NotImplementedError(f"{self.what} is training / dataset glue outside the MI355X hot path")


def build_model(args):
    """models/__init__.py:4-5 -> tce_rvos.build :638-719.  Returns (model, criterion, postprocessors)."""
    cfg = config_from_args(args)
    model = ReferFormer(cfg, args=args)
    from .criterion import build_criterion  # models/tce_rvos.py:686-715 (forward values; loads no library until it is called)
    from .postprocess import build_postprocessors  # models/tce_rvos.py:717-719
    return model, build_criterion(args), build_postprocessors(args, getattr(args, "dataset_file", None))
