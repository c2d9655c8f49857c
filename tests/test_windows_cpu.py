"""CPU: the context-frame window planner (video.plan_windows, plan_window_forwards, window_args) against a plain-loop restatement of
the reference's keep_fps / f_extra loop (tests/_windows.py)."""
import argparse

import pytest

from _windows import reference_windows
from tce_rvos_amd.video import plan_window_forwards, plan_windows, window_args


def _per_frame(plan):
    """(window number, clip position, clip ids) per written video frame, and the frames in writing order"""
    rows, order = {}, []
    for w, (ids, first, count, lo) in enumerate(plan):
        assert count >= 1 and 0 <= first and first + count <= len(ids), (w, ids, first, count)
        for j in range(count):
            assert lo + j not in rows, ("written twice", lo + j)
            rows[lo + j] = (w, first + j, ids)
            order.append(lo + j)
    return rows, order


CASES = [(N, n, e, last) for n in (1, 3, 5) for e in (0, 1, 2, 3) for last in ("short", "shifted")
         for N in range(1, 3 * n + 2) if last == "short" or N >= n]


def test_the_case_table_covers_what_it_says():
    assert len(CASES) == 4 * (sum(3 * n + 1 for n in (1, 3, 5)) + sum(3 * n + 1 - (n - 1) for n in (1, 3, 5)))
    assert (16, 5, 3, "shifted") in CASES and (1, 5, 3, "short") in CASES and (5, 5, 0, "shifted") in CASES


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("last", ["short", "shifted"])
def test_plan_equals_the_restated_reference_loop(n, last):
    for N, n_, e, last_ in CASES:
        if (n_, last_) != (n, last):
            continue
        want = reference_windows(N, n, e, last)
        plan = plan_windows(N, n, e, last, "leading")
        rows, order = _per_frame(plan)
        assert order == list(range(N)), (N, n, e, last, order)  # every frame exactly once, in increasing order
        assert [rows[f] for f in range(N)] == want, (N, n, e, last)
        assert len(plan) == len(range(0, N, n))
        centre = plan_windows(N, n, e, last, "centre")
        assert centre == [(ids, first + e, count, lo) for ids, first, count, lo in plan], (N, n, e, last)
        crow, corder = _per_frame(centre)
        assert corder == list(range(N))
        for f in range(N):  # the aligned variant writes each frame from itself
            assert crow[f][2][crow[f][1]] == f, (N, n, e, last, f)


def test_worked_example_short():
    plan = plan_windows(12, 5, 2)
    assert plan == [((0, 0, 0, 1, 2, 3, 4, 5, 6), 0, 5, 0), (tuple(range(3, 12)), 0, 5, 5), ((8, 9, 10, 11, 11, 11), 0, 2, 10)]
    src = [ids[first + j] for ids, first, count, _ in plan for j in range(count)]
    assert src == [0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    centre = plan_windows(12, 5, 2, take="centre")
    assert [ids[first + j] for ids, first, count, _ in centre for j in range(count)] == list(range(12))
    assert [w[1:] for w in centre] == [(2, 5, 0), (2, 5, 5), (2, 2, 10)]


def test_worked_example_shifted():
    plan = plan_windows(12, 5, 1, last="shifted")
    assert plan == [((0, 0, 1, 2, 3, 4, 5), 0, 5, 0), ((4, 5, 6, 7, 8, 9, 10), 0, 5, 5), ((6, 7, 8, 9, 10, 11, 11), 3, 2, 10)]
    assert plan_windows(12, 5, 1, last="shifted", take="centre")[2][1:] == (4, 2, 10)
    # a video that divides evenly has no shifted window
    assert plan_windows(10, 5, 1, last="shifted") == plan_windows(10, 5, 1, last="short")


@pytest.mark.parametrize("N,n", [(1, 3), (7, 3), (9, 3), (32, 32), (40, 32), (5, 1)])
def test_no_context_and_a_short_last_window_are_the_chunk_loop(N, n):
    plan = plan_windows(N, n, 0, "short")
    assert plan == [(tuple(range(lo, min(lo + n, N))), 0, min(lo + n, N) - lo, lo) for lo in range(0, N, n)]
    assert plan_windows(N, n, 0, "short", "centre") == plan


def test_forwards_of_two_shared_captions_and_one_alone():
    wins = plan_windows(7, 3, 1)
    assert [len(w[0]) for w in wins] == [5, 5, 3]
    fw = plan_window_forwards([9, 9, 6], wins, max_group=2)
    assert fw == [([0, 1], [0]), ([0, 1], [1]), ([0, 1], [2]), ([2], [0, 1]), ([2], [2])]
    # one window per forward; more captions than a group holds; a lone rest of a bucket
    fw = plan_window_forwards([9, 9, 9], wins, max_group=2, windows_per_forward=1)
    assert fw == [([0, 1], [0]), ([0, 1], [1]), ([0, 1], [2]), ([2], [0]), ([2], [1]), ([2], [2])]
    fw = plan_window_forwards([6, 9], wins, mixed_lengths=True)
    assert fw == [([0, 1], [0]), ([0, 1], [1]), ([0, 1], [2])]


@pytest.mark.parametrize("lengths,mg,wpf,mixed", [([9, 9, 6], 2, 4, False), ([5, 7, 5, 5, 7, 9], 2, 2, False), ([5, 7, 9], 4, 8, True),
                                                  ([4], 4, 3, False), ([4, 4, 4, 4, 4], 4, 1, False)])
@pytest.mark.parametrize("N,n,e,last", [(7, 3, 1, "short"), (23, 5, 2, "short"), (23, 5, 2, "shifted"), (4, 5, 3, "short")])
def test_every_caption_window_pair_runs_exactly_once(lengths, mg, wpf, mixed, N, n, e, last):
    wins = plan_windows(N, n, e, last)
    fw = plan_window_forwards(lengths, wins, mg, wpf, mixed)
    pairs = [(i, w) for caps, ws in fw for i in caps for w in ws]
    assert sorted(pairs) == [(i, w) for i in range(len(lengths)) for w in range(len(wins))]
    for caps, ws in fw:
        assert (len(caps) >= 2 and len(ws) == 1) or (len(caps) == 1 and 1 <= len(ws) <= wpf)
        assert len(caps) <= mg and len({len(wins[w][0]) for w in ws}) == 1
        assert mixed or len({lengths[i] for i in caps}) == 1
    for i in range(len(lengths)):  # a caption's windows come in order
        mine = [w for caps, ws in fw if i in caps for w in ws]
        assert mine == sorted(mine)


def test_window_args():
    assert window_args(argparse.Namespace(num_frames=6, f_extra=2)) == {"num_frames": 6, "f_extra": 2}
    assert window_args(argparse.Namespace(num_frames=5)) == {"num_frames": 5, "f_extra": 0}
    assert window_args(argparse.Namespace(num_frames=4, f_extra=0, keep_fps=True)) == {"num_frames": 4, "f_extra": 0}


@pytest.mark.parametrize("kw", [dict(num_frames=0), dict(num_frames=-2), dict(f_extra=-1), dict(last="long"), dict(take="center"),
                                dict(n_frames=0), dict(n_frames=4, last="shifted"), dict(n_frames=1, num_frames=2, last="shifted")])
def test_bad_arguments_raise(kw):
    args = dict(n_frames=12, num_frames=5, f_extra=1)
    args.update(kw)
    with pytest.raises(ValueError):
        plan_windows(**args)


def test_the_restatement_refuses_what_the_reference_leaves_undefined():
    with pytest.raises(ValueError):
        reference_windows(4, 5, 1, "shifted")
