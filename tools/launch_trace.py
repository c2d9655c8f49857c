"""The clip's launch program as text, for diffing two trees: per case and topology (the capture topology through
model.hazard_check, the eager single-arena one through forward_features / forward_group / forward_indexed inside
hazard.recording()) one line per recorded launch -- entry point, stream, vector clock (streams as ordinals by first appearance:
this pins every fork / join edge), read and write sets -- then the recorder's edges and host syncs.  A third recording per case,
" / replay", is one call of the public entry point that replays the case's captured graph: the launches around the graph launch
(inputs staged in, outputs copied out).  An interval inside one of the
pass's arenas prints as arena:offset+length (equal runs at one stride as arena:offset+length*count/stride); everything else
(weights, inputs: addresses differ between processes) as its total length.  Launch.site is left out.
    python tools/launch_trace.py [--root TREE] [--digest] [--only SUBSTRING] > trace.txt
--root: the tree whose package is traced (default: this one), so one file serves both sides of a comparison.
--digest: per recording the SHA-256 of its launch lines in their place (the form that is committed: the full trace is ten
thousand lines; two trees with equal digests have equal traces, and the full form shows where unequal ones part)."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--digest", action="store_true")
ap.add_argument("--only", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: E402
from tce_rvos_amd import build_model, hazard, load_synth_weights, ops  # noqa: E402

PAD = 1


def fmt_set(iv, arenas):
    """iv: merged [n, 2] intervals; arenas: [(base, end)] in ordinal order"""
    inside, ext = [], 0
    for lo, hi in iv.tolist():
        for k, (b, e) in enumerate(arenas):
            l2, h2 = max(lo, b), min(hi, e)
            if l2 < h2:
                inside.append((k, l2 - b, h2 - l2))
                ext -= h2 - l2
        ext += hi - lo
    inside.sort()  # by arena ordinal, then offset: not by where the allocator happened to place the arenas
    parts, i = [], 0
    while i < len(inside):  # equal runs at one stride -> one term
        k, off, n = inside[i]
        j = i + 1
        if j < len(inside) and inside[j][0] == k and inside[j][2] == n:
            st = inside[j][1] - off
            while j < len(inside) and inside[j] == (k, off + (j - i) * st, n):
                j += 1
        parts.append(f"{k}:{off}+{n}" + (f"*{j - i}/{st}" if j - i > 1 else ""))
        i = j
    return ",".join(parts + ([f"ext{ext}"] if ext else [])) or "-"


def dump(title, rec, arenas):
    arenas = [(int(t.data_ptr()), int(t.data_ptr()) + t.numel() * t.element_size()) for t in arenas]
    order = {}
    print(f"== {title}: {len(rec.launches)} launches, arenas {[e - b for b, e in arenas]}")
    lines = []
    for L in rec.launches:
        s = order.setdefault(L.stream, len(order))
        for t in L.clock:
            order.setdefault(t, len(order))
        clock = ",".join(f"{k}:{v}" for k, v in sorted((order[t], v) for t, v in L.clock.items()))
        lines.append(f"{L.name} s{s} [{clock}] r={fmt_set(L.reads, arenas)} w={fmt_set(L.writes, arenas)}\n")
    text = "".join(lines)
    print(f"sha256 {hashlib.sha256(text.encode()).hexdigest()} on {len(order)} streams\n" if a.digest else text, end="")
    print(f"edges {rec.edges} host_syncs {rec.host_syncs}")


def frames(T, H, W, seed):
    return torch.randn(T, 3, H, W, generator=torch.Generator().manual_seed(seed)).cuda()


def tokens(G, L, seed):
    return torch.randint(3, 50000, (G, L), generator=torch.Generator().manual_seed(seed)).cuda()


def ragged_ids(lens, seed):
    ids = torch.full((len(lens), max(lens)), PAD, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    for i, n in enumerate(lens):
        ids[i, :n] = torch.randint(3, 50000, (n,), generator=g)
        ids[i, 0], ids[i, n - 1] = 0, 2
    return ids.cuda()


# name: backbone, model flags, gemm mode, T (frames per clip), H, W, token ids, hazard_check / forward keywords
CASES = [
    ("swin-t T3 96x132 L32", "swin_t_p4w7", {}, None, 3, 96, 132, lambda: tokens(1, 32, 3), {}),
    ("swin-t T5 360x640 L32 (config 2)", "swin_t_p4w7", {}, None, 5, 360, 640, lambda: tokens(1, 32, 3), {}),
    ("swin-t T3 96x160 valid 90x140", "swin_t_p4w7", {}, None, 3, 96, 160, lambda: tokens(1, 32, 3), {"valid": (90, 140)}),
    ("swin-t T2 64x96 L40", "swin_t_p4w7", {}, None, 2, 64, 96, lambda: tokens(1, 40, 3), {}),
    ("video-swin-t T4 96x128 L9", "video_swin_t_p4w7", {}, None, 4, 96, 128, lambda: tokens(1, 9, 3), {}),
    ("resnet50 T1 96x128 L9", "resnet50", {}, None, 1, 96, 128, lambda: tokens(1, 9, 3), {}),
    ("group G2 T3 96x132 L9", "swin_t_p4w7", {}, None, 3, 96, 132, lambda: tokens(2, 9, 3), {"groups": 2}),
    ("shared G3 select (0,1,1)", "swin_t_p4w7", {}, None, 3, 96, 132, lambda: tokens(3, 9, 5),
     {"groups": 3, "shared": True, "select": (0, 1, 1)}),
    ("select 1 of T3, G1", "swin_t_p4w7", {}, None, 3, 96, 132, lambda: tokens(1, 9, 3), {"select": 1}),
    ("ragged G3 T3 96x132", "swin_t_p4w7", {}, None, 3, 96, 132, lambda: ragged_ids((32, 20, 11), 31), {"groups": 3, "ragged": True}),
    ("index 3 windows of a pool of 6", "swin_t_p4w7", {}, None, 6, 96, 132, lambda: tokens(3, 9, 601),
     {"index": [(0, 0, 1, 2), (1, 2, 3, 4), (3, 4, 5, 5)]}),
    ("swin-t T3 96x132 exact fp32", "swin_t_p4w7", {}, "f32", 3, 96, 132, lambda: tokens(1, 32, 3), {}),
    ("qtrans=False", "swin_t_p4w7", {"qtrans": False}, None, 3, 96, 132, lambda: tokens(1, 32, 3), {}),
    ("with_box_refine=False", "swin_t_p4w7", {"with_box_refine": False}, None, 3, 96, 132, lambda: tokens(1, 32, 3), {}),
]
models = {}


def model_of(backbone, flags, mode):
    key = (backbone, tuple(sorted(flags.items())))
    if key not in models:
        args = dict(backbone=backbone, with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8, qtrans=True,
                    num_feature_levels=4, text_encoder_layers=1)
        args.update(flags)
        m = build_model(argparse.Namespace(**args))[0].cuda().eval()
        load_synth_weights(m, 5)
        models[key] = m
    m = models[key]
    ops.set_gemm_mode(mode or "f16x3")
    m.repack()
    return m


def eager(model, name, T, H, W, x, ids, kw):
    """the same case through the public entry point: eagerly (use_graph off: one warm-up pass, one recorded pass, the slot's
    arena), then as a graph replay (graph_after = 1: the third call replays; the fourth is recorded).  tce_graph_launch is no
    launch to the recorder, so the replay's recording is what a replay launches OUTSIDE the graph -- the staging copy in, the
    output copy out -- with byte counts only (the graph's arenas are not listed)."""
    tgt = [{"size": torch.tensor([H, W])}]
    G = kw.get("groups", 1)
    if "index" in kw:
        run = lambda: model.forward_indexed(x, kw["index"], ids, tgt)  # noqa: E731
    elif G > 1:
        clips = [x] * G if kw.get("shared") else list(x.split(T))
        tg = [dict(tgt[0], valid_indices=torch.tensor([v])) for v in kw["select"]] if "select" in kw else tgt
        run = lambda: model.forward_group(clips, ids, tg, ragged=kw.get("ragged", False))  # noqa: E731
    else:
        hid, pooled = model.forward_text_encoder(ids, "cuda")
        run = lambda: model.forward_features(x, hid[0], pooled[0], H, W, valid_hw=kw.get("valid"), select=kw.get("select"))  # noqa: E731
    model.use_graph = False
    try:
        run()
        torch.cuda.synchronize()
        sd = model._text_plan().sd
        with hazard.recording(tables=[sd["embeddings.word_embeddings.weight"], sd["embeddings.position_embeddings.weight"]]) as rec:
            run()
        torch.cuda.synchronize()
    finally:
        model.use_graph = True
    dump(name + " / eager", rec, [model._arenas[0].buf])
    n_graphs, model.graph_after = len(model._graphs), 1
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    assert len(model._graphs) == n_graphs + 1, "the case was not captured: its fourth call would not be a replay"
    with hazard.recording(tables=[sd["embeddings.word_embeddings.weight"], sd["embeddings.position_embeddings.weight"]]) as rec:
        run()
    torch.cuda.synchronize()
    dump(name + " / replay", rec, [])


with torch.no_grad():
    for name, backbone, flags, mode, T, H, W, ids_of, kw in CASES:
        if a.only not in name:
            continue
        model = model_of(backbone, flags, mode)
        G = 1 if kw.get("shared") or "index" in kw else kw.get("groups", 1)
        x, ids = frames(T * G, H, W, 11), ids_of()

        def observe(when, res, rec, name=name):
            if when == "after":
                dump(name + " / capture", rec, [r.buf for r in res if isinstance(r, ops.Arena)])
        rep = model.hazard_check(x, ids, (H, W), observe=observe, **kw)
        print(rep if not rep.clean else f"race free, {rep.unordered_pairs} unordered pairs compared")
        eager(model, name, T, H, W, x, ids, kw)
        sys.stdout.flush()
ops.set_gemm_mode("f16x3")
