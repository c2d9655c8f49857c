"""CPU: model._dispatch, the one place where a launch program runs as eager launches, is captured or is replayed.  With _run,
_capture and ops.copy_many replaced it is host logic: when a key is captured (sightings, use_graph, keys pinned to the eager
path), how a replay stages the frame sources into the static frame buffer (one copy launch, destinations at the sources'
cumulative row offsets, the other statics behind them), that the statics never alias a caller's tensor, and the LRU order of the
graph cache (through the real _capture, on stand-ins for the graph objects of torch.cuda)."""
import argparse
import contextlib
from collections import OrderedDict

import pytest
import torch

from tce_rvos_amd import model as M
from tce_rvos_amd import ops

H, W = 4, 6


@pytest.fixture(scope="module")
def built():
    from tce_rvos_amd import build_model
    args = argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)
    m, _, _ = build_model(args)
    return m.eval()


def compute(frames, text):
    """What the stand-in program returns: per-frame values, so a row staged to the wrong place or not at all shows."""
    per = frames.flatten(1).sum(1) + text.sum().to(torch.float32)
    return {"pred_masks": per * torch.arange(1, frames.shape[0] + 1), "aux_outputs": [{"pred_masks": frames.flatten(1)[:, 0] - per}]}


class Rig:
    def __init__(self, model):
        self.model, self.eager, self.captures, self.copies = model, 0, 0, []

    def dispatch(self, key, sources, ids, **kw):
        return self.model._dispatch(key, sources, (ids,), lambda i: i, float(H), float(W), (1, ids.shape[1]), 0, **kw)


@pytest.fixture()
def rig(built, monkeypatch):
    r = Rig(built)
    for name, fresh in (("_graphs", OrderedDict()), ("_sightings", OrderedDict()), ("_nograph", set()), ("use_graph", True),
                        ("graph_after", 1), ("max_graphs", 6)):
        monkeypatch.setattr(built, name, fresh)

    def run(frames, text, img_h, img_w, res, slot=0, **kw):
        r.eager += res is None
        return compute(frames, text)

    def capture(key, statics, fn, like, slot=0, text=None):
        r.captures += 1
        res = M._Resources(*[None] * 9)
        out = fn(res)

        class Exe:
            @staticmethod
            def replay():
                for dst, src in zip(M._flat_outputs(out), M._flat_outputs(fn(res))):
                    dst.copy_(src)
        ent = built._graphs[key] = M._Entry(Exe(), statics, out, res, 0, None)
        return ent

    def copy_many(dsts, srcs):
        r.copies.append((list(dsts), list(srcs)))
        for d, s in zip(dsts, srcs):
            d.copy_(s)

    monkeypatch.setattr(built, "_run", run)
    monkeypatch.setattr(built, "_capture", capture)
    monkeypatch.setattr(ops, "copy_many", copy_many)
    return r


def frames_of(rows, seed):
    return torch.randint(-8, 9, (rows, 3, H, W), generator=torch.Generator().manual_seed(seed)).to(torch.float32)


IDS = torch.arange(3, 8)[None]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(M._flat_outputs(a), M._flat_outputs(b))) and list(a) == list(b)


def test_sightings_decide_between_eager_capture_and_replay(rig):
    x = frames_of(3, 1)
    want = compute(x, IDS)
    assert same(rig.dispatch(("k",), [x], IDS), want)
    assert (rig.eager, rig.captures, len(rig.copies)) == (1, 0, 0) and not rig.model._graphs  # first sighting: eager, no capture
    assert same(rig.dispatch(("k",), [x], IDS), want)
    assert (rig.eager, rig.captures, len(rig.copies)) == (1, 1, 1) and list(rig.model._graphs) == [("k",)]  # captured and replayed
    assert same(rig.dispatch(("k",), [x], IDS), want)
    assert (rig.eager, rig.captures, len(rig.copies)) == (1, 1, 2)  # replayed, not captured again


def test_use_graph_off_never_captures(rig):
    rig.model.use_graph = False
    x = frames_of(3, 2)
    for _ in range(4):
        assert same(rig.dispatch(("k",), [x], IDS), compute(x, IDS))
    assert (rig.eager, rig.captures, rig.copies) == (4, 0, []) and not rig.model._graphs


def test_a_capture_that_gives_up_pins_the_key_to_the_eager_path(rig, monkeypatch):
    attempts = []

    def capture(key, statics, fn, like, slot=0, text=None):
        attempts.append(key)
        rig.model._nograph.add(key)

    monkeypatch.setattr(rig.model, "_capture", capture)
    for n in range(1, 5):
        x = frames_of(3, 10 + n)
        assert same(rig.dispatch(("k",), [x], IDS), compute(x, IDS))
        assert rig.eager == n
    assert attempts == [("k",)] and rig.copies == [] and not rig.model._graphs


LAYOUTS = {
    "one source of 3 rows": (lambda: [frames_of(3, 3)], [0]),
    "a group of 3 clips of 2 rows": (lambda: [frames_of(2, 4), frames_of(2, 5), frames_of(2, 6)], [0, 2, 4]),
    "runs (0, 2) and (4, 1) of a pool of 6": (lambda: (lambda pool: [pool[0:2], pool[4:5]])(frames_of(6, 7)), [0, 2]),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_replay_stages_the_sources_into_their_rows_with_one_copy(rig, layout):
    make, offsets = LAYOUTS[layout]
    sources, ids = make(), IDS.clone()
    rig.dispatch(("k",), sources, ids)
    rig.dispatch(("k",), sources, ids)   # captured and replayed
    assert rig.captures == 1 and len(rig.copies) == 1
    for s in sources:                    # new values in the caller's tensors (in place: the pool's runs stay views of the pool)
        s.mul_(-3).add_(1)
    ids += 2
    del rig.copies[:]
    got = rig.dispatch(("k",), sources, ids)
    assert rig.captures == 1 and rig.eager == 1 and len(rig.copies) == 1  # exactly one copy_many call per replay
    dsts, srcs = rig.copies[0]
    ent = rig.model._graphs[("k",)]
    buf = ent.statics[0]
    assert tuple(buf.shape) == (sum(s.shape[0] for s in sources), 3, H, W) and buf.is_contiguous()
    assert len(dsts) == len(sources) + 1 and len(srcs) == len(dsts)
    for d, s, off in zip(dsts, sources, offsets):
        assert d.data_ptr() == buf[off].data_ptr() and d.shape == s.shape and d.is_contiguous()
    assert dsts[-1] is ent.statics[1] and all(a is b for a, b in zip(srcs, sources + [ids]))
    assert same(got, compute(torch.cat(sources, 0), ids))  # the replay is the eager pass of the new values
    assert all(g is not o for g, o in zip(M._flat_outputs(got), M._flat_outputs(ent.out)))  # handed back as fresh tensors


def test_the_static_frame_buffer_never_aliases_the_callers_tensor(rig):
    x = frames_of(3, 8)  # fp32 and contiguous: the eager frame tensor IS x
    rig.dispatch(("k",), [x], IDS)
    rig.dispatch(("k",), [x], IDS)
    ent = rig.model._graphs[("k",)]
    held = ent.statics[0].clone()
    assert torch.equal(held, x) and ent.statics[0].data_ptr() != x.data_ptr()
    x.add_(5)
    assert torch.equal(ent.statics[0], held)
    assert ent.statics[1].data_ptr() != IDS.data_ptr()


def test_lru_evicts_the_oldest_entry_and_a_replay_renews_one(built, monkeypatch):
    """Through the real _capture: the graph objects of torch.cuda and the arenas are stand-ins, the cache logic is the model's."""
    class Graph:
        def replay(self):
            pass

    rig = Rig(built)
    for name, fresh in (("_graphs", OrderedDict()), ("_sightings", OrderedDict()), ("_nograph", set()), ("graph_after", 0),
                        ("max_graphs", 2), ("use_graph", True)):
        monkeypatch.setattr(built, name, fresh)
    monkeypatch.setattr(built, "_run", lambda frames, text, *a, **k: compute(frames, text))
    monkeypatch.setattr(built, "_branch_resources", lambda like, slot=0, text=None: M._Resources(*[None] * 9))
    monkeypatch.setattr(ops, "copy_many", lambda dsts, srcs: [d.copy_(s) for d, s in zip(dsts, srcs)])
    monkeypatch.setattr(M, "GRAPH_OWN_EXEC", False)
    monkeypatch.setattr(M, "COPYPLAN", False)
    monkeypatch.setattr(M, "_ALL_GRAPHS", [])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
    monkeypatch.setattr(torch.cuda, "graph", lambda g, **k: contextlib.nullcontext())
    x = frames_of(2, 9)
    for k in "ab":
        rig.dispatch((k,), [x], IDS)
    assert list(rig.model._graphs) == [("a",), ("b",)]
    rig.dispatch(("a",), [x], IDS)                      # a replay moves its key to the end ...
    assert list(rig.model._graphs) == [("b",), ("a",)]
    rig.dispatch(("c",), [x], IDS)                      # ... so the third key evicts "b", the oldest
    assert list(rig.model._graphs) == [("a",), ("c",)]
    assert len(M._ALL_GRAPHS) == 3                      # executables of the never-destroy path outlive their entries
