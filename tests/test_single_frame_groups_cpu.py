"""CPU: the host side of A2D-Sentences / JHMDB-Sentences clip groups -- the planner of video.run_annotated_frames, the copy table of a
group's single-frame selection (pipeline.pick_segments), and the group output stage's cap, host structure
and access model (include/tce_rvos_eval.h)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "tce_a2d_group_masks_u8"


@pytest.fixture(scope="module")
def built_lib():
    from tce_rvos_amd import build as b
    return b.build(verbose=False)


# ------------------------------------------------------------------------------------------------------------------ planner
def _sample_set():
    a, b = (3, 3, 96, 132), (3, 3, 96, 128)
    shapes = [a, b, a, a, b, a, a, a, b, a]
    indices = [1, 1, 1, 0, 1, 1, 0, 1, 2, 1]
    lengths = [5, 5, 7, 5, 5, 5, 5, 5, 5, 5]
    return shapes, indices, lengths


@pytest.mark.parametrize("max_group", [1, 2, 3, 8])
@pytest.mark.parametrize("mixed", [False, True])
def test_plan_is_a_partition_in_first_sighting_order_within_the_cap(max_group, mixed):
    from tce_rvos_amd.video import plan_single_frame_groups
    shapes, indices, lengths = _sample_set()
    plan = plan_single_frame_groups(shapes, indices, lengths, max_group=max_group, mixed_lengths=mixed)
    flat = [i for g in plan for i in g]
    assert sorted(flat) == list(range(len(shapes))) and len(flat) == len(set(flat))          # every sample exactly once
    assert all(1 <= len(g) <= max_group for g in plan)
    key = (lambda i: (shapes[i], indices[i])) if mixed else (lambda i: (shapes[i], indices[i], lengths[i]))
    assert all(len({key(i) for i in g}) == 1 for g in plan)                                  # one bucket per group
    assert all(g == sorted(g) for g in plan)                                                 # input order inside a group
    firsts = []                                                                              # buckets in order of first sighting
    for g in plan:
        if key(g[0]) not in firsts:
            firsts.append(key(g[0]))
    seen = []
    for i in range(len(shapes)):
        if key(i) not in seen:
            seen.append(key(i))
    assert firsts == seen
    # a bucket's groups are consecutive, and all but its last are full
    for k in seen:
        own = [g for g in plan if key(g[0]) == k]
        at = plan.index(own[0])
        assert plan[at:at + len(own)] == own and all(len(g) == max_group for g in own[:-1])


def test_plan_buckets_by_index_and_by_length_and_mixed_lengths_merges():
    from tce_rvos_amd.video import plan_single_frame_groups
    shapes, indices, lengths = _sample_set()
    assert plan_single_frame_groups(shapes, indices, lengths, max_group=8) == [[0, 5, 7, 9], [1, 4], [2], [3, 6], [8]]
    assert plan_single_frame_groups(shapes, indices, lengths, max_group=3) == [[0, 5, 7], [9], [1, 4], [2], [3, 6], [8]]
    assert plan_single_frame_groups(shapes, indices, lengths, max_group=8, mixed_lengths=True) == [[0, 2, 5, 7, 9], [1, 4], [3, 6], [8]]
    assert plan_single_frame_groups([], [], []) == []
    with pytest.raises(ValueError):
        plan_single_frame_groups(shapes, indices[:-1], lengths)


# ------------------------------------------------------------------------------------------------------------ pick_segments
def _emulate(maps, table):
    """the segment copy restated with numpy: per level, the segments back to back"""
    out = []
    for m, segs in zip(maps, table):
        assert all(rw == m.shape[1] for _, _, rw in segs)
        out.append(np.concatenate([m[off:off + rows] for off, rows, _ in segs], 0))
    return out


@pytest.mark.parametrize("G,Tc,idx", [(3, 3, (1, 0, 2)), (2, 4, (3, 0)), (4, 3, (0, 2, 1, 1)), (17, 2, tuple(i % 2 for i in range(17)))])
def test_pick_segments_is_the_index_select_of_each_clips_frame(G, Tc, idx):
    from tce_rvos_amd.pipeline import pick_segments
    sizes, chs = [(6, 7), (3, 4), (2, 2), (1, 1)], [8, 16, 32, 64]
    rng = np.random.default_rng(3)
    maps = [rng.standard_normal((G * Tc * h * w, c)).astype(np.float32) for (h, w), c in zip(sizes, chs)]
    table = pick_segments(G, Tc, idx, sizes, chs)
    assert len(table) == 4 and all(len(segs) == G for segs in table)
    for (h, w), c, m, got in zip(sizes, chs, maps, _emulate(maps, table)):
        frames = torch.from_numpy(m).view(G * Tc, h * w, c)
        want = frames.index_select(0, torch.tensor([g * Tc + idx[g] for g in range(G)])).reshape(G * h * w, c).numpy()
        assert got.shape == (G * h * w, c) and np.array_equal(got, want)


def test_pick_segments_shared_form_reads_the_one_clip():
    from tce_rvos_amd.pipeline import pick_segments
    G, Tc, idx = 3, 3, (0, 1, 1)
    sizes, chs = [(5, 3), (3, 2), (2, 1), (1, 1)], [4, 8, 16, 32]
    rng = np.random.default_rng(4)
    maps = [rng.standard_normal((Tc * h * w, c)).astype(np.float32) for (h, w), c in zip(sizes, chs)]       # ONE clip's frames
    table = pick_segments(G, Tc, idx, sizes, chs, shared=True)
    for (h, w), c, m, got in zip(sizes, chs, maps, _emulate(maps, table)):
        want = torch.from_numpy(m).view(Tc, h * w, c).index_select(0, torch.tensor(idx)).reshape(G * h * w, c).numpy()
        assert np.array_equal(got, want)
        assert all(off + rows <= Tc * h * w for off, rows, _ in table[sizes.index((h, w))])


def test_pick_segments_rejects_bad_indices():
    from tce_rvos_amd.pipeline import pick_segments
    sizes, chs = [(2, 2)] * 4, [4] * 4
    with pytest.raises(IndexError):
        pick_segments(2, 3, (0, 3), sizes, chs)
    with pytest.raises(IndexError):
        pick_segments(2, 3, (-1, 0), sizes, chs)
    with pytest.raises(ValueError):
        pick_segments(2, 3, (0,), sizes, chs)


# ---------------------------------------------------------------------------------------------- the group entry and its model
# (symbols, binding table, exports, argtypes, models / launch-free names of include/tce_rvos_eval.h: tests/test_host_cpu.py)
def test_the_group_cap_and_the_host_structure_are_the_headers():
    from tce_rvos_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "tce_rvos_eval.h")).read()
    cap = int(re.search(r"#define\s+TCE_A2D_GROUP_MAX\s+(\d+)", text).group(1))
    assert cap == _lib.A2D_GROUP_MAX == ops.A2D_GROUP_MAX
    assert ctypes.sizeof(_lib.A2dGroupSample) == 56 and cap * 56 == 896


def test_access_model_on_a_hand_made_table_and_under_the_recording_proxy():
    """Two samples of N = 3 queries and 4 x 6 mask planes with different frame sizes; the second's logits are 2 floats apart, so
    they show up as three separate 4-byte intervals; the outputs start on odd and on even-but-unaligned addresses."""
    from tce_rvos_amd import _lib, hazard
    table = (_lib.A2dGroupSample * 2)()
    a, b = table
    a.masks, a.logits, a.out, a.scores = 0x100000, 0x200000, 0x300001, 0x400000
    a.fh, a.fw, a.H0, a.W0, a.logit_stride = 13, 20, 9, 11, 1
    b.masks, b.logits, b.out, b.scores = 0x110000, 0x210004, 0x310002, 0x410000
    b.fh, b.fw, b.H0, b.W0, b.logit_stride = 16, 24, 20, 30, 2
    reads = [[0x100000, 0x100120], [0x110000, 0x110120], [0x200000, 0x20000C],
             [0x210004, 0x210008], [0x21000C, 0x210010], [0x210014, 0x210018]]
    writes = [[0x300001, 0x30012A], [0x310002, 0x31070A], [0x400000, 0x40000C], [0x410000, 0x41000C]]
    rd, wr = hazard.MODELS[ENTRY]((table, 2, 3, 4, 6, 0.5, 0))
    assert hazard.union(*rd).tolist() == reads and hazard.union(*wr).tolist() == writes
    rd, wr = hazard.MODELS[ENTRY]((table, 1, 3, 4, 6, 0.5, 0))  # B decides how much of the table counts
    assert hazard.union(*rd).tolist() == [reads[0], reads[2]] and hazard.union(*wr).tolist() == [writes[0], writes[2]]

    class StandIn:
        def __getattr__(self, name):
            return lambda *a: name
    rec = hazard.Recorder()
    proxy = hazard._LibProxy(StandIn(), rec, dry=True)
    assert getattr(proxy, ENTRY)(table, 2, 3, 4, 6, 0.5, 0) == 0
    assert [x.name for x in rec.launches] == [ENTRY]
    assert rec.launches[0].reads.tolist() == reads and rec.launches[0].writes.tolist() == writes
    assert proxy.tce_rle_ws_bytes(3, 9, 11) == "tce_rle_ws_bytes" and len(rec.launches) == 1  # a query: passed through


def test_bad_calls_are_rejected_before_anything_is_launched(built_lib):
    from tce_rvos_amd import _lib
    l = _lib.lib()
    f = getattr(l, ENTRY)
    assert f(None, 1, 5, 4, 6, 0.5, None) != 0 and (ENTRY + ": null").encode() in l.tce_last_error()
    table = (_lib.A2dGroupSample * 1)()
    assert f(table, 0, 5, 4, 6, 0.5, None) != 0 and b"samples per launch" in l.tce_last_error()
    assert f(table, _lib.A2D_GROUP_MAX + 1, 5, 4, 6, 0.5, None) != 0 and b"samples per launch" in l.tce_last_error()
    assert f(table, 1, 0, 4, 6, 0.5, None) != 0 and b"extent" in l.tce_last_error()
    assert f(table, 1, 5, 4, 6, 0.5, None) != 0 and b"null pointer in sample 0" in l.tce_last_error()
    e = table[0]
    e.masks, e.logits, e.out, e.scores = 4096, 8192, 12289, 16384   # never dereferenced: every call below is rejected on the host
    e.fh, e.fw, e.H0, e.W0, e.logit_stride = 17, 24, 8, 10, 1
    assert f(table, 1, 5, 4, 6, 0.5, None) != 0 and b"4x" in l.tce_last_error()
    e.fh, e.logit_stride = 16, 0
    assert f(table, 1, 5, 4, 6, 0.5, None) != 0 and b"extent in sample 0" in l.tce_last_error()
    e.logit_stride, e.H0, e.W0 = 1, 40000, 40000
    assert f(table, 1, 5, 4, 6, 0.5, None) != 0 and b"2^31" in l.tce_last_error()
    e.H0, e.W0, e.scores = 8, 10, 16386
    assert f(table, 1, 5, 4, 6, 0.5, None) != 0 and b"aligned" in l.tce_last_error()
