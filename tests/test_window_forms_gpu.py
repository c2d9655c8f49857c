"""GPU: every launch form of the Swin and Video-Swin window attention (W1..W6 of tests/_window.py, each in every arithmetic mode it
runs in; the cores W1..W5 on every design, the fused W6 on N, G+, G- and U) against the fp64 reference built from the oracle's
geometry functions, element by element, under the derived bound of tests/_arith.py with no margin -- at the smallest frame
sizes that reach each edge of the window geometry (one real token in a padded window, H <= shift, an odd window count, shrunken
3-D windows, one ragged key tile, an un-ragged last tile, 13 key tiles),
and on operands that let the finite -100 mask lose (G+) or hold (G-), make the running maximum rise or fall in every key tile (R^,
Rv) and count the keys (U).  tests/test_window_forms_cpu.py shows that plain fp32 torch is inside these bounds on these inputs and
that each of twelve planted defects is outside them.

The output buffer holds a NaN pattern before every launch; no element is skipped.  Every case appends (form, mode, case, design,
max err / B) to a table the last test writes to profiles/r33_window_forms.txt."""
import os

import pytest
import torch

import _window as Wn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r33_window_forms.txt")
RESULTS = []
NAN_BITS = 0x7FC0DEAD


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tce_rvos_amd import ops as _ops
    return _ops


@pytest.fixture
def lib():
    from tce_rvos_amd._lib import lib as _lib
    return _lib()


@pytest.fixture(autouse=True)
def _range_flag_stays_clean(ops):
    """No design is meant to leave the fp16 range (the largest operand is a k component of 130 / (8 * 32^-0.5) = 92): the flag is
    clean before and after every test."""
    ops.check_range()
    yield
    ops.check_range()


def dev(t):
    return t.cuda().contiguous()


def _bits(t):
    return t.view(torch.int32)


def _nan_filled(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def case_name(lay):
    return f"{lay.kind} {lay.T}x{lay.H}x{lay.W} " + (f"shift={lay.shift}" if lay.kind == "2d" else f"shifted={bool(lay.shift)}")


def run_core(ops, lib, entry, dbg, mode, lay, qkv, qb, table, nh):
    """One call of ops.window_attn / ops.window_attn3d under the debug switch `dbg` (restored to 1) in `mode`, into a NaN-patterned
    buffer -> out on the host.  Asserts the form the call is meant to select and that the operands are unchanged bit for bit."""
    C = 32 * nh
    ins = [dev(qkv), dev(qb), dev(table)]
    before = [t.clone() for t in ins]
    out = _nan_filled(lay.ntok, C)
    lib.tce_debug_window_attn_set_mfma(dbg)
    try:
        with ops.arith(mode):
            if entry == "2d":
                ops.window_attn(*ins, lay.T, lay.H, lay.W, C, nh, lay.shift, out=out)
            else:
                ops.window_attn3d(*ins, lay.T, lay.H, lay.W, C, nh, bool(lay.shift), out=out)
        torch.cuda.synchronize()
    finally:
        lib.tce_debug_window_attn_set_mfma(1)
    for t, b in zip(ins, before):
        assert torch.equal(_bits(t), _bits(b)), f"{case_name(lay)} [{mode}]: an operand was written"
    return out.cpu()


def check(form, mode, case, design, out, ref, B, rows=None):
    """Per-element |out - ref| <= B over the whole output; records the case.  For a coded design the message names the key that won:
    rows(t) = the attention rows behind t (the identity for the cores)."""
    r = Wn.ratio(out, ref, B)
    i = int(r.argmax())
    rB = float(r.flatten()[i])
    RESULTS.append((form, mode, case, design, rB))
    print(f"{form} [{mode}] {case} {design}: err/B {rB:.3g}")
    if rB > 1.0:
        row, col = divmod(i, ref.shape[-1])
        msg = (f"{form} [{mode}] {case} {design}: {int((r > 1.0).sum())} of {r.numel()} elements outside the bound; worst err/B = {rB:.3g} "
               f"(out {float(out.flatten()[i]):.6e}, ref {float(ref.flatten()[i]):.6e}) at token {row}, head {col // 32}, channel {col % 32}")
        if design in Wn.CODED and rows is not None:
            h = col // 32
            won = [Wn.decode(rows(t)[row, 32 * h:32 * h + 32]) for t in (out, ref)]
            msg += f"; head {h} of the row sits on key {won[0]}, the reference on key {won[1]}"
        raise AssertionError(msg)
    return rB


_SHARED = {}


def reference(lay, design, nh, mode):
    """(operands, ref, B) of a case, computed once per product bound and left unchanged."""
    key = (lay.kind, lay.T, lay.H, lay.W, lay.shift, design, nh)
    if key not in _SHARED:
        _SHARED[key] = (Wn.operands(design, lay, nh), {})
    operands, by = _SHARED[key]
    p = Wn.PRODUCT[mode].__name__
    if p not in by:
        by[p] = Wn.core_ref_and_bound(lay, *operands, nh, mode)[:2]
    return operands, by[p][0], by[p][1]


def run_forms(ops, lib, lay, design, nh):
    outs = {}
    for form, entry, dbg, modes in Wn.FORM_RUNS:
        if entry != lay.kind:
            continue
        for mode in modes:
            assert Wn.window_form(entry, mode, dbg) == form
            operands, ref, B = reference(lay, design, nh, mode)
            out = run_core(ops, lib, entry, dbg, mode, lay, *operands, nh)
            check(form, mode + ("" if dbg == 1 else f" dbg={dbg}"), case_name(lay), design, out, ref, B, rows=lambda t: t)
            outs[(form, dbg, mode)] = out
    return outs


CASES_2D = [c + (s,) for c, _ in Wn.CASES_2D for s in (0, 3)]
CASES_3D = [c for c, _ in Wn.CASES_3D]


@pytest.mark.parametrize("T,H,W,shift", CASES_2D)
def test_forms_cases_2d(ops, lib, T, H, W, shift):
    """W1, W2 (as mode f32 and as dbg = 2) and W3 (both split modes) at every 2-D case, design N; the exact kernel gives the same
    bits whichever way it was selected, and W1 / W2 agree within the sum of their bounds."""
    lay = Wn.layout("2d", T, H, W, shift)
    outs = run_forms(ops, lib, lay, "N", Wn.heads_2d(T, H, W))
    assert torch.equal(_bits(outs[("W2", 1, "f32")]), _bits(outs[("W2", 2, "f16x3")])), "W2: mode f32 and dbg = 2 differ"
    _, ref, B = reference(lay, "N", Wn.heads_2d(T, H, W), "f32")
    agree("W1", outs[("W1", 0, "f16x3")], "W2", outs[("W2", 1, "f32")], B, B, case_name(lay))


@pytest.mark.parametrize("T,H,W,shifted", CASES_3D)
def test_forms_cases_3d(ops, lib, T, H, W, shifted):
    """W4 (as mode f32 and as dbg = 0) and W5 (both split modes) at every 3-D case, design N; W4's two selections give the same
    bits, and W4 / W5 in f16x3 agree within the sum of their bounds."""
    lay = Wn.layout("3d", T, H, W, shifted)
    outs = run_forms(ops, lib, lay, "N", 2)
    assert torch.equal(_bits(outs[("W4", 1, "f32")]), _bits(outs[("W4", 0, "f16x3")])), "W4: mode f32 and dbg = 0 differ"
    _, ref, B = reference(lay, "N", 2, "f16x3")
    agree("W4", outs[("W4", 0, "f16x3")], "W5", outs[("W5", 1, "f16x3")], B, B, case_name(lay))


def agree(fa, a, fb, b, Ba, Bb, case):
    d = (a.double() - b.double()).abs().nan_to_num(nan=float("inf"))
    r = float(torch.where(d == 0, torch.zeros_like(d), d / (Ba + Bb)).max())
    print(f"{fa} against {fb} {case}: |a - b| / (Ba + Bb) {r:.3g}")
    assert r <= 1.0, f"{fa} against {fb} {case}: worst |a - b| / (Ba + Bb) = {r:.3g}"


DESIGN_RUNS = Wn.design_runs()
# no (core form, design) pair may drop out because a case does not take the design
assert {(k, d) for d, k, *_ in DESIGN_RUNS} == {(k, d) for k in ("2d", "3d") for d in Wn.DESIGNS if d != "N"}


@pytest.mark.parametrize("design,kind,T,H,W,shift", DESIGN_RUNS)
def test_forms_designs(ops, lib, design, kind, T, H, W, shift):
    """W1..W5, each in every mode it runs in, on G+ and G- (at the cases with a window of two regions of real tokens: two 2-D,
    two 3-D), R^, Rv and U (at every case of _window.DESIGN_CASES)."""
    lay = Wn.layout(kind, T, H, W, shift)
    run_forms(ops, lib, lay, design, Wn.heads_2d(T, H, W) if kind == "2d" else 2)


# ---------------------------------------------------------------------------------------------------------------
# W6: the fused half-block
# ---------------------------------------------------------------------------------------------------------------
TRAIL = 3   # rows behind the output that must stay as they were


def run_fused(ops, mode, lay, C, x, g1, b1, wqkv, bqkv, table, wp, bp, inplace=False):
    """One launch in `mode` with x at a pitch of C + 4 (the gap columns hold NaN) and out at a pitch of C + 8 inside a NaN-patterned
    buffer with TRAIL rows behind it, which must come back bit-identical outside the output columns.  inplace: out = x (its pitch)."""
    M = lay.ntok
    with ops.arith(mode):
        pk = ops.swin_attn_pack(dev(wqkv), dev(wp))
        xb = _nan_filled(M, C + 4)
        xb[:, :C] = dev(x)
        keep = xb.clone()
        args = (pk, dev(bqkv), dev(bp), dev(table), dev(g1), dev(b1), lay.T, lay.H, lay.W, C, lay.shift)
        if inplace:
            ops.swin_attn_fused(xb[:, :C], *args)
            torch.cuda.synchronize()
            assert torch.equal(_bits(xb[:, C:]), _bits(keep[:, C:])), "in place: a gap column of x was written"
            return xb[:, :C].cpu()
        ob = _nan_filled(M + TRAIL, C + 8)
        ops.swin_attn_fused(xb[:, :C], *args, out=ob[:M, :C])
        torch.cuda.synchronize()
    assert torch.equal(_bits(xb), _bits(keep)), "x was written"
    res = ob[:M, :C].cpu()
    _bits(ob)[:M, :C] = NAN_BITS
    assert bool((_bits(ob) == NAN_BITS).all()), "wrote outside its output columns"
    return res


FUSED_CASES = [(C,) + thw + (s,) for C in Wn.FUSED_C for thw in Wn.CASES_FUSED[C] for s in (0, 3)]


@pytest.mark.parametrize("C,T,H,W,shift", FUSED_CASES)
def test_fused_cases(ops, C, T, H, W, shift):
    """W6 at three cases per C, design N, in the three modes; mode f32 is not rejected: the entry reads only the single-pass
    switch, so it runs the three-product arithmetic of f16x3 -- the same bits, held to the same bound."""
    lay = Wn.layout("2d", T, H, W, shift)
    operands = Wn.fused_operands("N", lay, C)
    outs = {}
    for mode in Wn.MODES:
        outs[mode] = run_fused(ops, mode, lay, C, *operands)
        assert bool(torch.isfinite(outs[mode]).all())
        ref, B, _ = Wn.fused_ref_and_bound(lay, *operands, mode)
        check("W6", mode, f"C={C} " + case_name(lay), "N", outs[mode], ref, B)
    assert Wn.window_form("fused", "f32") == "W6"
    assert torch.equal(_bits(outs["f32"]), _bits(outs["f16x3"])), "W6: mode f32 is not the arithmetic of f16x3"


@pytest.mark.parametrize("C", Wn.FUSED_C)
@pytest.mark.parametrize("design", [d for d in Wn.FUSED_DESIGNS if d != "N"])
def test_fused_designs(ops, C, design):
    """G+, G- and U through LayerNorm and the projection, at the three-window case and the case with H < 7, shifted."""
    for thw in Wn.CASES_FUSED[C][:2]:
        lay = Wn.layout("2d", *thw, 3)
        assert Wn.design_applies(design, lay)
        operands = Wn.fused_operands(design, lay, C)
        for mode in Wn.SPLIT_MODES:
            ref, B, _ = Wn.fused_ref_and_bound(lay, *operands, mode)
            x, wp, bp = operands[0], operands[6], operands[7]
            check("W6", mode, f"C={C} " + case_name(lay), design, run_fused(ops, mode, lay, C, *operands), ref, B,
                  rows=lambda t: Wn.fused_attention_of(t, x, wp, bp))


@pytest.mark.parametrize("C", Wn.FUSED_C)
def test_fused_in_place(ops, C):
    """out = x gives the bits of the out-of-place call (every workgroup reads its windows' rows before it writes them, and no
    other workgroup reads them), at the three-window case whose last workgroup holds one window."""
    lay = Wn.layout("2d", 1, 7, 15, 3)
    operands = Wn.fused_operands("N", lay, C)
    for mode in Wn.SPLIT_MODES:
        a = run_fused(ops, mode, lay, C, *operands)
        b = run_fused(ops, mode, lay, C, *operands, inplace=True)
        assert torch.equal(_bits(a), _bits(b)), f"W6 C={C} [{mode}]: in place differs from out of place"


def test_zz_write_profile(ops):
    """Writes the table of every case above (run the whole module: each test appends its lines)."""
    best = {}
    for form, mode, case, design, rB in RESULTS:
        best[(form, mode, case, design)] = max(best.get((form, mode, case, design), 0.0), rB)
    ran = {(f, m.split()[0]) for f, m, _, _ in best}
    need = {(f, m) for f, _, _, modes in Wn.FORM_RUNS for m in modes} | {("W6", "f32")}
    core = {"2d": ("W1", "W2", "W3"), "3d": ("W4", "W5")}
    pairs = {(f, d) for f, _, _, d in best}
    missing = {(f, d) for k in core for f in core[k] for d in Wn.DESIGNS} | {("W6", d) for d in Wn.FUSED_DESIGNS}
    assert missing <= pairs, f"(form, design) pairs that did not run: {sorted(missing - pairs)}"
    assert need <= ran, f"forms that did not run: {sorted(need - ran)}"
    assert all(r <= 1.0 for r in best.values())
    with open(PROFILE, "w") as f:
        f.write("# tests/test_window_forms_gpu.py on an MI355X: per (launch form, arithmetic mode, case, operand design), the largest\n"
                "# |out - fp64 ref| over the whole output as a fraction of the derived bound B (no margin).  Forms W1..W6 and the designs:\n"
                "# tests/_window.py.  'dbg=' is the value given to tce_debug_window_attn_set_mfma (W1 / W4 outside mode f32, W2 in a\n"
                "# split mode).  W6 in mode f32 runs the arithmetic of f16x3 (asserted bit for bit).\n"
                "# No kernel was changed: every ratio below is of the kernels as they were.\n"
                "# form | mode | case | design | max err/B\n")
        for (form, mode, case, design), rB in sorted(best.items()):
            f.write(f"{form} | {mode} | {case} | {design} | {rB:.3f}\n")
