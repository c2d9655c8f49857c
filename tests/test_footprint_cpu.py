"""The footprint harness (tests/_footprint.py) can fail, and its coverage cannot rot.

CPU slabs, plain torch functions standing in for kernels, hand-made interval sets standing in for access models: each
defect a kernel or a model can have is planted once and must be reported for the stated reason; the correct stand-in
passes.  The second half checks the GPU module's case table against hazard.MODELS and _lib.SIGNATURES."""
import ctypes

import numpy as np
import pytest
import torch

import _footprint as fp
from tce_rvos_amd import _lib, hazard

ROWS, COLS, PITCH = 5, 6, 8
GUARD = 4096  # the stand-ins stray by a few bytes; the 256 KiB condition of the GPU cases is checked on its own below


def _standin(defect=None, model_bias=True, ws_hole=False, ws_read=False):
    """out[r, :] = 2 * x[r, :] + bias  on pitched rows, with one planted defect."""
    st = {}

    def build(S):
        x = S.randn("x", (ROWS, COLS), pitch=PITCH)
        bias = S.randn("bias", (COLS,))
        out = S.alloc("out", (ROWS, COLS), pitch=PITCH)
        ws = S.alloc("ws", (16,))
        st.update(x=x, bias=bias, out=out, ws=ws, S=S)

        def fn():
            keep = out[3, 2].clone()
            out.copy_(2 * x + bias)
            ws[:15 if ws_hole else 16] = 1.0
            flat = S.mem[S.buf("out").off:].view(torch.float32)
            xflat = S.mem[S.buf("x").off:].view(torch.float32)
            if defect == "past_last_row":
                flat[(ROWS - 1) * PITCH + COLS + (PITCH - COLS)] = 7.0  # first element of row ROWS
            elif defect == "pad_column":
                flat[1 * PITCH + COLS] = 7.0
            elif defect == "guard_before":
                S.mem[S.buf("out").off - 1] = 7
            elif defect == "writes_input":
                x[2, 3] = 7.0
            elif defect == "skips_output":
                out[3, 2] = keep  # what the slab held before the run
            elif defect == "zero_times_pad":
                out[0, 0] += 0.0 * xflat[COLS]          # the pad column right of x[0, :]
            elif defect == "reads_unwritten_ws":
                out[0, 0] += ws[15]                     # with ws_hole: a workspace word this launch never produced
            elif defect == "max_with_pad":
                out[0, 0] = torch.maximum(out[0, 0], xflat[COLS])
        return fn

    def model():
        F = 4
        S = st["S"]
        base = S.base
        rd = [hazard.strided(base + S.buf("x").off, COLS * F, (ROWS, PITCH * F))]
        if model_bias:
            rd.append(hazard.dense(base + S.buf("bias").off, COLS * F))
        wr = [hazard.strided(base + S.buf("out").off, COLS * F, (ROWS, PITCH * F)), hazard.dense(base + S.buf("ws").off, 16 * F)]
        if ws_read:  # a workspace the model lists as read AND written (split-K partial sums, GroupNorm statistics)
            rd.append(wr[1])
        return rd, wr

    def record(fn, dry):
        if not dry:
            fn()
        return model()
    return build, record


def _run(props="WOR", exempt=("ws",), **kw):
    build, record = _standin(**kw)
    return fp.check_case(fp.Slab(1 << 18, guard_min=GUARD), build, record, exempt=exempt, props=props, label="standin")


def test_correct_standin_passes_all_three():
    info = _run()
    assert info["W"] == 2 and info["O"] == 2 and info["R"] == 3
    assert info["written_bytes"] == ROWS * COLS * 4 + 64 and info["read_bytes"] == ROWS * COLS * 4 + COLS * 4
    assert info["guard_bytes"] >= 5 * GUARD and info["pad_bytes"] == 2 * (ROWS - 1) * (PITCH - COLS) * 4


@pytest.mark.parametrize("defect,where", [
    ("past_last_row", f"after the end of out"),
    ("pad_column", f"out + {(1 * PITCH + COLS) * 4} bytes (row 1, byte {COLS * 4}"),
    ("guard_before", "guard 1 bytes before out"),
    ("writes_input", f"x + {(2 * PITCH + 3) * 4} bytes (row 2, byte 12"),
])
def test_w_reports_a_stray_write_with_buffer_and_offset(defect, where):
    with pytest.raises(fp.FootprintError) as e:
        _run(props="W", defect=defect)
    assert "W violated" in str(e.value) and where in str(e.value), str(e.value)


def test_o_reports_a_hole_and_exempts_only_declared_workspaces():
    with pytest.raises(fp.FootprintError) as e:
        _run(props="O", defect="skips_output")
    assert "O violated" in str(e.value) and f"out + {(3 * PITCH + 2) * 4} bytes (row 3" in str(e.value), str(e.value)
    # the same hole inside a declared workspace passes ...
    assert _run(props="O", ws_hole=True)["O"] == 2
    # ... and fails when the buffer is not declared
    with pytest.raises(fp.FootprintError) as e:
        _run(props="O", ws_hole=True, exempt=())
    assert "O violated" in str(e.value) and "ws + 60 bytes" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,fills", [
    ({"defect": "zero_times_pad"}, {"qnan"}),          # 0 * NaN = NaN; 0 * -1e38 = -0.0 adds nothing: the NaN fill sees it
    ({"defect": "max_with_pad"}, {"qnan"}),            # torch.maximum propagates NaN; a NaN-dropping v_min is the test below
    ({"model_bias": False}, {"qnan", "big"}),
])
def test_r_reports_a_dependence_on_unmodelled_bytes(kw, fills):
    seen = set()
    for fname, word in fp.FILLS[1:]:
        build, record = _standin(**kw)
        S = fp.Slab(1 << 18, guard_min=GUARD)
        old = fp.FILLS
        fp.FILLS = (old[0], (fname, word))
        try:
            fp.check_case(S, build, record, exempt=("ws",), props="R", label="standin")
        except fp.FootprintError as e:
            assert "R violated" in str(e) and f"'{fname}' fill" in str(e) and "out + 0 bytes" in str(e), str(e)
            seen.add(fname)
        finally:
            fp.FILLS = old
    print(f"{kw}: R failed under {sorted(seen)}")
    assert seen == fills


def test_r_fills_declared_workspaces_even_where_the_model_lists_them_as_read():
    kw = dict(defect="reads_unwritten_ws", ws_hole=True, ws_read=True)
    build, record = _standin(**kw)
    # without the declaration the workspace keeps its zero base content in all three runs: the stale read is invisible
    assert fp.check_case(fp.Slab(1 << 18, guard_min=GUARD), build, record, exempt=("ws",), props="R")["R"] == 3
    build, record = _standin(**kw)
    with pytest.raises(fp.FootprintError) as e:
        fp.check_case(fp.Slab(1 << 18, guard_min=GUARD), build, record, exempt=("ws",), scratch=("ws",), props="R", label="standin")
    assert "R violated" in str(e.value) and "out + 0 bytes" in str(e.value), str(e.value)
    # a correct launch with a partly written, read-listed workspace passes: its unwritten words are not results
    build, record = _standin(ws_hole=True, ws_read=True)
    assert fp.check_case(fp.Slab(1 << 18, guard_min=GUARD), build, record, exempt=("ws",), scratch=("ws",), props="R")["R"] == 3


def test_r_large_fill_catches_a_max_that_drops_nan():
    """v_max / v_min return the other operand for a NaN: a stand-in with that behaviour passes the NaN fill and is caught by
    the large finite one only when the stray term can win -- which is why the pattern is large in magnitude AND the module
    also runs the zero fill (the reference the other two are compared with)."""
    def build(S):
        x = S.rand("x", (ROWS, COLS), lo=-3.0, hi=-1.0, pitch=PITCH)
        out = S.alloc("out", (ROWS, COLS), pitch=PITCH)

        def fn():
            pad = S.mem[S.buf("x").off:].view(torch.float32)[COLS]
            out.copy_(x)
            out[0, 0] = torch.fmin(x[0, 0], pad)  # fmin drops NaN, as v_min does
        fn.S = S
        return fn

    def record(fn, dry):
        if not dry:
            fn()
        S = fn.S
        return ([hazard.strided(S.base + S.buf("x").off, COLS * 4, (ROWS, PITCH * 4))],
                [hazard.strided(S.base + S.buf("out").off, COLS * 4, (ROWS, PITCH * 4))])
    old = fp.FILLS
    try:
        fp.FILLS = old[:2]
        assert fp.check_case(fp.Slab(1 << 18, guard_min=GUARD), build, record, props="R")["R"] == 2   # zero + NaN: not seen
        fp.FILLS = old
        with pytest.raises(fp.FootprintError) as e:
            fp.check_case(fp.Slab(1 << 18, guard_min=GUARD), build, record, props="R")
        assert "'big' fill" in str(e.value)
    finally:
        fp.FILLS = old


def test_ranges_outside_the_slab_are_an_error_not_ignored():
    build, record = _standin()

    def rec2(fn, dry):
        rd, wr = record(fn, dry)
        return rd + [hazard.dense(1 << 20, 64)], wr  # an address that is no buffer of the case
    with pytest.raises(fp.FootprintError) as e:
        fp.check_case(fp.Slab(1 << 18, guard_min=GUARD), build, rec2, exempt=("ws",), label="standin")
    assert "forgot a buffer" in str(e.value)


def test_guards_and_pitches_meet_the_stated_condition():
    S = fp.Slab(16 << 20)
    S.begin(fp.CANARIES[0])
    a = S.alloc("a", (7, 100), pitch=104)
    b = S.alloc("b", (2, 3, 4000), pitch=4096, bstride=3 * 4096 + 64)
    c = S.alloc("c", (10,), dtype=torch.uint8)
    prev_end = 0
    for buf in S.bufs:
        need = max(fp.GUARD_MIN, fp.GUARD_ROWS * buf.pitch_bytes)
        assert buf.off - prev_end >= need and buf.off % fp.ALIGN == 0
        prev_end = buf.off + buf.nbytes
    assert S.used - prev_end >= fp.GUARD_MIN
    assert a.stride() == (104, 1) and b.stride() == (3 * 4096 + 64, 4096, 1) and c.numel() == 10
    assert bool((S.words[:S.used // 4] == fp._i32(fp.CANARIES[0])).all())
    iv = np.array([[10, 20], [40, 44]])
    comp = S.complement(iv)
    assert comp.tolist() == [[0, 10], [20, 40], [44, S.used]]
    m = S.mask(iv)
    assert int(m.sum()) == 14 and bool(m[10]) and not bool(m[20]) and bool(m[43])


def test_windowed_walk_of_an_arena_finds_the_one_stray_byte():
    buf = torch.empty(1000, dtype=torch.uint8)
    buf.view(torch.int32).fill_(fp._i32(fp.CANARIES[0]))
    base = buf.data_ptr()
    writes = np.array([[base + 100, base + 228], [base + 256, base + 512], [base + 900, base + 2000]])
    buf[100:228] = 0
    buf[256:512] = 1
    buf[900:] = 2
    for window in (64, 256, 4096):
        assert fp.first_touched_outside(buf, writes, fp.CANARIES[0], window) is None
    buf[515] ^= 0xFF
    for window in (64, 256, 4096):
        assert fp.first_touched_outside(buf, writes, fp.CANARIES[0], window) == (515, 1)


# ---------------------------------------------------------------------------------------------------------------------
# coverage of the GPU module's case table
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_exactly_the_modelled_entry_points():
    import test_footprint_gpu as g
    names = {}
    for c in g.CASES:
        names[c.entry] = names.get(c.entry, 0) + 1
    # the main header's models; the output stages' are held to their kernels by their own tests (test_label_objects_gpu.py,
    # test_a2d_post_gpu.py, test_jf_score_gpu.py, test_a2d_score_gpu.py, test_png_gpu.py, test_png_dyn_gpu.py,
    # test_a2d_group_post_gpu.py, test_vis_overlay_gpu.py, test_png_rgb_gpu.py, test_png_file_gpu.py, test_refexp_gpu.py)
    main = set(hazard.MODELS) & set(_lib.SIGNATURES)
    assert set(hazard.MODELS) - main == {"tce_label_objects_u8", "tce_a2d_masks_u8", "tce_rle_counts_u32", "tce_jf_counts_i32",
                                         "tce_rle_decode_u8", "tce_mask_overlap_i32", "tce_png_deflate_u8", "tce_png_deflate_dyn_u8",
                                         "tce_a2d_group_masks_u8", "tce_vis_overlay_u8", "tce_png_filter_rgb_u8",
                                         "tce_png_deflate_rows_u8", "tce_png_file_u8", "tce_refexp_group_u8", "tce_refexp_giou_f32"}
    assert set(names) == main, (sorted(main - set(names)), sorted(set(names) - main))
    few = {n: k for n, k in names.items() if k < 2}
    assert not few, f"entry points with fewer than two cases: {few}"
    ids = [c.id for c in g.CASES]
    assert len(ids) == len(set(ids))


def test_exemption_lists_name_pointer_arguments_of_their_entry_points():
    import test_footprint_gpu as g
    assert not getattr(g, "W_EXEMPT", None)  # W has no exemptions at all
    for table in (g.O_EXEMPT, g.ATOMIC, g.HOST_ARGS):
        for entry, args in table.items():
            assert entry in hazard.MODELS, entry
            argtypes = _lib.SIGNATURES[entry][1]
            for name, idx in args.items():
                assert isinstance(name, str) and 0 <= idx < len(argtypes), (entry, name, idx)
                t = argtypes[idx]
                assert t is _lib.c_f or (isinstance(t, type) and issubclass(t, ctypes._Pointer)), (entry, name, idx, t)
    # the lists stay short: workspaces / counters only
    assert sum(len(v) for v in g.O_EXEMPT.values()) <= 12 and len(g.ATOMIC) <= 2
    used = {(c.entry, n) for c in g.CASES for n in c.exempt}
    assert used == {(e, n) for e, a in g.O_EXEMPT.items() for n in a}, "an O exemption no case uses, or a case exempting an unlisted buffer"
