"""Host side of the clip groups over a frame pool (model.forward_indexed): pipeline.pool_segments against a per-frame restatement,
video.plan_window_forwards(share="frames") / video.window_pool against plan_windows, and the argument errors that are raised before
any launch.  No GPU."""
import argparse
import random

import pytest
import torch

from tce_rvos_amd.pipeline import pool_segments
from tce_rvos_amd.video import plan_expression_groups, plan_window_forwards, plan_windows, window_pool

SIZES = [(6, 9), (3, 5), (2, 3), (1, 2)]
CHANNELS = [4, 8, 16, 32]


# ------------------------------------------------------------------------------------------------------------- pool_segments
def restated(index, unit):
    """(backbone frames, per slot frame its position among them): one frame at a time, nothing merged"""
    index = [tuple(t) for t in index]
    if unit == "frame":
        frames = sorted(set(f for t in index for f in t))
        where = [frames.index(f) for t in index for f in t]
    else:
        clips = []
        for t in index:
            if t not in clips:
                clips.append(t)
        frames = [f for t in clips for f in t]
        where = [clips.index(t) * len(t) + j for t in index for j in range(len(t))]
    return frames, where


def apply_table(src, segments, rows):
    """what ops.copy_row_segments does, on the host: the segments back to back"""
    if not segments:
        return src
    out = torch.cat([src[off:off + n] for off, n, _ in segments], 0)
    assert out.shape[0] == rows
    return out


def hold(index, unit):
    frames, table = pool_segments(index, SIZES, CHANNELS, unit)
    want_frames, where = restated(index, unit)
    assert list(frames) == want_frames
    assert len(table) == len(SIZES)
    slots = len(index) * len(index[0])
    for (h, w), c, segs in zip(SIZES, CHANNELS, table):
        hw = h * w
        src = torch.arange(len(frames) * hw * c).view(len(frames) * hw, c)  # the backbone's map
        want = torch.cat([src[p * hw + r:p * hw + r + 1] for p in where for r in range(hw)], 0)  # row by row
        got = apply_table(src, segs, slots * hw)
        assert torch.equal(got, want), (index, unit, hw)
        if segs:  # whole rows inside the source; the destination covered exactly once, in order; merged as far as possible
            assert all(rw == c and n >= 1 and 0 <= off and off + n <= src.shape[0] for off, n, rw in segs)
            assert sum(n for _, n, _ in segs) == slots * hw
            assert all(a[0] + a[1] != b[0] for a, b in zip(segs, segs[1:])), "consecutive rows left unmerged"
        else:
            assert where == list(range(slots)) and len(frames) == slots
    assert all(bool(t) == bool(table[0]) for t in table)
    return frames, table


@pytest.mark.parametrize("unit", ["frame", "clip"])
def test_pool_segments_equal_the_per_frame_restatement_on_random_indices(unit):
    rng = random.Random(19)
    for _ in range(200):
        F, Tc, G = rng.randint(1, 9), rng.randint(1, 4), rng.randint(1, 8)
        hold([tuple(rng.randrange(F) for _ in range(Tc)) for _ in range(G)], unit)


@pytest.mark.parametrize("unit", ["frame", "clip"])
def test_pool_segments_named_cases(unit):
    # all frames distinct and in order: the identity has no segments
    frames, table = hold([(0, 1, 2), (3, 4, 5)], unit)
    assert frames == [0, 1, 2, 3, 4, 5] and table == [[], [], [], []]
    # the same clip three times: one backbone clip, one segment per slot
    frames, table = hold([(2, 3, 4)] * 3, unit)
    assert frames == [2, 3, 4] and [len(t) for t in table] == [3] * 4
    assert table[0] == [(0, 3 * 54, 4)] * 3
    # a frame repeated inside one clip
    frames, table = hold([(0, 0, 0, 1, 2), (1, 2, 3, 4, 4)], unit)
    if unit == "frame":
        assert frames == [0, 1, 2, 3, 4] and len(table[0]) == 5  # 0 | 0 | 0 1 2 | 1 2 3 4 | 4
    else:
        assert frames == [0, 0, 0, 1, 2, 1, 2, 3, 4, 4] and table[0] == []  # two distinct clips in order: nothing to gather
    # more than 16 segments (one tce_copy_segments launch holds 16)
    frames, table = hold([(4, 2, 0), (5, 3, 1)] * 4, unit)
    assert len(table[0]) == (24 if unit == "frame" else 4)  # frame by frame; (clip A, clip B) four times over
    frames, table = hold([(0, 1, 2), (5, 3, 1), (5, 3, 1)] * 9, unit)
    assert len(table[0]) > 16


def test_distinct_clips_come_in_first_appearance_order():
    frames, _ = pool_segments([(7, 8), (1, 2), (7, 8), (0, 0), (1, 2)], SIZES, CHANNELS, "clip")
    assert frames == [7, 8, 1, 2, 0, 0]
    frames, _ = pool_segments([(7, 8), (1, 2), (7, 8), (0, 0), (1, 2)], SIZES, CHANNELS, "frame")
    assert frames == [0, 1, 2, 7, 8]


def test_pool_segments_rejects_what_it_cannot_plan():
    for bad in ([], [()], [(0, 1), (2,)], [(0, -1)]):
        with pytest.raises(ValueError):
            pool_segments(bad, SIZES, CHANNELS, "frame")
    with pytest.raises(ValueError):
        pool_segments([(0, 1)], SIZES, CHANNELS, "window")


# ------------------------------------------------------------------------------------------- plan_window_forwards(share="frames")
def todays_rule(lengths, windows, max_group=4, windows_per_forward=4, mixed_lengths=False):
    """plan_window_forwards as it stood before `share` existed, copied literally"""
    wpf = max(1, int(windows_per_forward))
    runs = []
    for w, win in enumerate(windows):
        if runs and len(runs[-1]) < wpf and len(windows[runs[-1][0]][0]) == len(win[0]):
            runs[-1].append(w)
        else:
            runs.append([w])
    out = []
    for grp in plan_expression_groups(lengths, max_group, mixed_lengths):
        if len(grp) >= 2:
            out += [(list(grp), [w]) for w in range(len(windows))]
        else:
            out += [(list(grp), list(r)) for r in runs]
    return out


LENGTHS = ([9], [9, 9], [9, 9, 6], [6, 9, 9, 14, 14])


def videos():
    for n in (1, 3, 5):
        for e in (0, 1, 2):
            for last in ("short", "shifted"):
                for N in range(1, 3 * n + 2):
                    if last == "shifted" and N < n:
                        continue
                    yield N, n, e, last


@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("max_pairs", [1, 4, 8])
@pytest.mark.parametrize("mixed", [False, True])
def test_frame_sharing_plan(lengths, max_pairs, mixed):
    for N, n, e, last in videos():
        wins = plan_windows(N, n, e, last)
        fw = plan_window_forwards(lengths, wins, mixed_lengths=mixed, share="frames", max_pairs=max_pairs)
        pairs = [(i, w) for caps, ws in fw for i in caps for w in ws]
        assert sorted(pairs) == [(i, w) for i in range(len(lengths)) for w in range(len(wins))]  # every pair exactly once
        interior = {}
        for caps, ws in fw:
            assert len(caps) * len(ws) <= max_pairs or len(ws) == 1
            assert len(ws) == max(1, max_pairs // len(caps)) or ws[-1] == len(wins) - 1 or \
                len(wins[ws[-1] + 1][0]) != len(wins[ws[0]][0])  # a full run, unless the windows or their length run out
            assert ws == list(range(ws[0], ws[0] + len(ws)))  # consecutive windows
            assert len({len(wins[w][0]) for w in ws}) == 1  # one clip length per forward
            assert mixed or len({lengths[i] for i in caps}) == 1
            pool, index = window_pool(wins, ws, len(caps))
            assert pool == sorted(set(pool)) and set(pool) == {f for w in ws for f in wins[w][0]}
            assert len(index) == len(caps) * len(ws)
            for c in range(len(caps)):  # caption-major slots; materialised, a slot's tuple is its window's ids
                for k, w in enumerate(ws):
                    assert tuple(pool[p] for p in index[c * len(ws) + k]) == wins[w][0]
            # a forward none of whose windows is clamped, shifted or short, with a full run of windows
            if len(ws) == max(1, max_pairs // len(caps)) and \
                    all(wins[w][0] == tuple(range(w * n - e, w * n + n + e)) for w in ws):
                interior.setdefault(tuple(caps), set()).add(tuple(index))
        assert all(len(v) == 1 for v in interior.values()), (N, n, e, last, interior)  # ONE relative pattern per bucket


@pytest.mark.parametrize("lengths,mg,wpf,mixed", [([9, 9, 6], 2, 4, False), ([5, 7, 5, 5, 7, 9], 2, 2, False), ([5, 7, 9], 4, 8, True),
                                                  ([4], 4, 3, False), ([4, 4, 4, 4, 4], 4, 1, False), ([9], 4, 4, False)])
def test_the_default_plan_is_what_it_was(lengths, mg, wpf, mixed):
    for N, n, e, last in videos():
        wins = plan_windows(N, n, e, last)
        want = todays_rule(lengths, wins, mg, wpf, mixed)
        assert plan_window_forwards(lengths, wins, mg, wpf, mixed) == want
        assert plan_window_forwards(lengths, wins, mg, wpf, mixed, share="clips", max_pairs=1) == want
    with pytest.raises(ValueError):
        plan_window_forwards([9], plan_windows(7, 3, 1), share="windows")


def test_worked_example_of_a_shared_pool():
    wins = plan_windows(12, 5, 1)
    assert [w[0] for w in wins] == [(0, 0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9, 10), (9, 10, 11, 11)]
    fw = plan_window_forwards([9, 9], wins, share="frames", max_pairs=4)
    assert fw == [([0, 1], [0, 1]), ([0, 1], [2])]
    pool, index = window_pool(wins, [0, 1], 2)
    assert pool == list(range(11))
    assert index == [(0, 0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9, 10)] * 2
    assert window_pool(wins, [2], 2) == ([9, 10, 11], [(0, 1, 2, 2)] * 2)
    # 14 frames through the backbone at 4 slots of 7; the default plan runs 2 x 7 + 4 for the same pairs, one window at a time


# ----------------------------------------------------------------------------------------------- forward_indexed: argument errors
@pytest.fixture(scope="module")
def model():
    from tce_rvos_amd import build_model
    args = argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                              qtrans=True, num_feature_levels=4, text_encoder_layers=1)
    m, _, _ = build_model(args)
    return m.eval()


def test_forward_indexed_rejects_bad_arguments_before_any_launch(model):
    from tce_rvos_amd.model import NestedTensor
    H, W = 32, 48
    pool = torch.zeros(4, 3, H, W)
    ids = torch.randint(3, 50000, (2, 5))
    tgt = [{"size": torch.tensor([H, W])}]
    good = [(0, 1), (2, 3)]
    with pytest.raises(ValueError, match="valid_indices"):
        model.forward_indexed(pool, good, ids, [{"size": torch.tensor([H, W]), "valid_indices": torch.tensor(0)}])
    with pytest.raises(ValueError, match="outside the pool"):
        model.forward_indexed(pool, [(0, 1), (2, 4)], ids, tgt)
    with pytest.raises(ValueError, match="outside the pool"):
        model.forward_indexed(pool, [(0, 1), (-1, 3)], ids, tgt)
    with pytest.raises(ValueError, match="one length"):
        model.forward_indexed(pool, [(0, 1), (2,)], ids, tgt)
    with pytest.raises(ValueError, match="G <= 64"):
        model.forward_indexed(pool, [(0, 1)] * 65, torch.randint(3, 50000, (65, 5)), tgt)
    with pytest.raises(ValueError, match="captions"):
        model.forward_indexed(pool, good, ids[:1], tgt)
    with pytest.raises(ValueError, match="captions"):
        model.forward_indexed(pool, good, ["a", "b", "c"], tgt)
    with pytest.raises(NotImplementedError, match="un-padded"):
        model.forward_indexed(NestedTensor(pool[None], torch.zeros(1, 4, H, W, dtype=torch.bool)), good, ids, tgt)
    with pytest.raises(ValueError):
        model.forward_indexed(pool[0], good, ids, tgt)
    with pytest.raises(RuntimeError, match="GPU"):  # every argument is fine: only now does the device matter
        model.forward_indexed(pool, good, ids, tgt)
