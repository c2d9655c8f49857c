"""GPU: every launch form of the generic attention core (tce_mha_f32 / tce_mha_ws_f32: F1..F7 of tests/_attn.py, each in every
arithmetic mode it has) against the fp64 reference over the kept keys, element by element, under the derived bound of
tests/_arith.py with no margin -- on key masks that leave whole tiles, the first tile or a whole KSPLIT wave at the sentinel, on
scores that make the running maximum rise or fall in every tile or saturate to one-hot, and in the memory layouts the pipeline
passes.  tests/test_attn_forms_cpu.py shows that plain fp32 torch is inside these bounds on these inputs and that a leaked key, a
mask applied to the wrong batch entry, a dropped tile and a wrong merge weight are outside them.

The reference and the bound are evaluated in fp64 on the device (the same formulas: _arith.on); no element is skipped.  Every case
appends (form, mode, family, max err / B, max err / S) to a table the last test writes to profiles/r27_attn_forms.txt."""
import os

import pytest
import torch

import _arith as A
import _attn as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r27_attn_forms.txt")
RESULTS = []
NOTES = []
NO_CLEAN_FLAG = {"test_nonfinite_k_at_masked_keys"}   # polls the flag itself
NAN_BITS = 0x7FC0DEAD


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tce_rvos_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _range_flag_stays_clean(ops, request):
    if request.node.originalname in NO_CLEAN_FLAG:
        yield
        return
    ops.check_range()
    yield
    ops.check_range()   # no case may raise the range flag


def _alloc(n):
    return torch.empty(n, dtype=torch.float32, device="cuda")


def _bits(t):
    return t.view(torch.int32)


def _nan_filled(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def launch(ops, c, mode, q, k, v, mask, layout="plain", Lk=None):
    """One call of ops.mha_core in `mode` and `layout` -> out [batch, Lq, E] (a contiguous copy).  Asserts the form the call is meant
    to select, that Q, K and V are unchanged bit for bit, and for L3 that the buffer around the output is."""
    name, batch, nh, Lq, Lk0, ws, _ = c
    Lk = Lk0 if Lk is None else Lk          # fewer keys than the K / V buffers hold (form agreement)
    E = nh * 32
    if Lk == Lk0:
        assert T.mha_form(batch, nh, Lq, Lk, mode, ws) == name[:2], (name, mode)
    km = None if mask is None else mask.cuda().contiguous()
    assert km is None or km.shape == (batch, Lk)
    dq, dk, dv = q.cuda().contiguous(), k.cuda().contiguous(), v.cuda().contiguous()
    Lkb = dk.shape[1]
    kw = dict(kmask=km, alloc=_alloc if ws else None)
    with ops.arith(mode):
        if layout in ("plain", "L3"):
            ins = (dq, dk, dv)
            before = [t.clone() for t in ins]
            if layout == "plain":
                out = _nan_filled(batch, Lq, E)
                ops.mha_core(dq, dk, dv, batch, nh, Lq, Lk, E, E, E, Lq * E, Lkb * E, Lkb * E, out, E, Lq * E, **kw)
                res = out
            else:   # the output inside a wider buffer, 16 bytes into it; everything around it must stay as it was
                ldo = E + 32
                buf = _nan_filled(4 + batch * Lq * ldo + 4)
                ops.mha_core(dq, dk, dv, batch, nh, Lq, Lk, E, E, E, Lq * E, Lkb * E, Lkb * E, buf[4:], ldo, Lq * ldo, **kw)
                body = buf[4:4 + batch * Lq * ldo].view(batch, Lq, ldo)
                res = body[..., :E].clone()
                _bits(body)[..., :E] = NAN_BITS
                assert bool((_bits(buf) == NAN_BITS).all()), f"{name} [{mode}] L3: wrote outside its output columns"
        elif layout == "L1":   # packed qk rows of 2E floats, K = Q + E; V separate
            Lm = max(Lq, Lkb)
            qk = _nan_filled(batch, Lm, 2 * E)
            qk[:, :Lq, :E], qk[:, :Lkb, E:] = dq, dk
            ins = (qk, dv)
            before = [t.clone() for t in ins]
            res = _nan_filled(batch, Lq, E)
            ops.mha_core(qk, qk[:, :, E:], dv, batch, nh, Lq, Lk, 2 * E, 2 * E, E, Lm * 2 * E, Lm * 2 * E, Lkb * E, res, E, Lq * E, **kw)
        elif layout == "L2":   # sequence-first: the batch stride is smaller than the row stride, for q, k, v and out
            Lm = max(Lq, Lkb)
            qk = _nan_filled(Lm, batch, 2 * E)
            qk[:Lq, :, :E], qk[:Lkb, :, E:] = dq.transpose(0, 1), dk.transpose(0, 1)
            vt = dv.transpose(0, 1).contiguous()
            ins = (qk, vt)
            before = [t.clone() for t in ins]
            out = _nan_filled(Lq, batch, E)
            ops.mha_core(qk, qk[:, :, E:], vt, batch, nh, Lq, Lk, batch * 2 * E, batch * 2 * E, batch * E, 2 * E, 2 * E, E, out, batch * E, E, **kw)
            res = out.transpose(0, 1).contiguous()
        else:
            raise ValueError(layout)
    torch.cuda.synchronize()
    for t, b in zip(ins, before):
        assert torch.equal(_bits(t), _bits(b)), f"{name} [{mode}] {layout}: an input was written"
    return res


def check(c, mode, family, out, ref, B, S, rows=None):
    """Per-element |out - ref| <= B over the whole output (rows: a batch-entry selection); records the case."""
    if rows is not None:
        out, ref, B, S = out[rows], ref[rows], B[rows], S[rows]
    r = T.ratio(out, ref, B)
    err = (out.double() - ref).abs().nan_to_num(nan=float("inf"))
    rS = float((err / S.clamp_min(1e-300)).max())
    i = int(r.argmax())
    rB = float(r.flatten()[i])
    RESULTS.append((c[0][:2], mode, family, rB, rS))
    print(f"{c[0]} [{mode}] {family}: err/B {rB:.3g} err/S {rS:.3g}")
    if rB > 1.0:
        E = ref.shape[-1]
        b, rem = divmod(i, ref.shape[-2] * E)
        row, col = divmod(rem, E)
        raise AssertionError(f"{c[0]} [{mode}] {family}: {int((r > 1.0).sum())} of {r.numel()} elements outside the bound; worst err/B = "
                             f"{rB:.3g} (out {float(out.flatten()[i]):.6e}, ref {float(ref.flatten()[i]):.6e}) at entry {b}, query {row}, "
                             f"head {col // 32}, channel {col % 32}")
    return rB


_SHARED = {}


def reference(c, design, mname, build, mode, share=False):
    """(q, k, v, mask, ref, B, S) of a case; share: kept for the other tests that use the same family (never modified)."""
    name, batch, nh, Lq, Lk, _, _ = c
    product = T.PRODUCT[mode]
    key = (name, design, mname, product.__name__)
    if key in _SHARED:
        return _SHARED[key]
    mask = build(batch, Lk)
    q, k, v = T.operands(design, batch, nh, Lq, Lk, mask=mask)
    val = (q, k, v, mask) + T.masked_ref_and_bound(q, k, v, mask, nh, product=product, device="cuda")
    if share:
        _SHARED[key] = val
    return val


PRIMARY = {c[0]: c for c in T.PRIMARY}
BOUNDARY = {c[0]: c for c in T.BOUNDARY}
FORM_MASKS = [(f, m) for f in PRIMARY for m in T.MASKS] + [(f, m) for f in ("F5", "F6") for m in T.MASKS_M4]


@pytest.mark.parametrize("form,mname", FORM_MASKS)
def test_forms_masks(ops, form, mname):
    """Every form in each of its modes at N(0, 1) under M0 (none), M1, M2, M3, M5, M6; the KSPLIT forms also under M4."""
    c = PRIMARY[form]
    build = dict(T.MASKS, **T.MASKS_M4)[mname]
    for mode in c[6]:
        q, k, v, mask, ref, B, S = reference(c, "N", mname, build, mode, share=(mname == "M2"))
        check(c, mode, f"N {mname}", launch(ops, c, mode, q, k, v, mask), ref, B, S)


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_threshold_cases(ops, name):
    """The shapes on either side of the 4096-tile, 256-key, 1024-key and workspace thresholds, under M2."""
    c = BOUNDARY[name]
    for mode in c[6]:
        q, k, v, mask, ref, B, S = reference(c, "N", "M2", T.mask_m2, mode)
        check(c, mode, "N M2 (threshold)", launch(ops, c, mode, q, k, v, mask), ref, B, S)


@pytest.mark.parametrize("form", list(PRIMARY))
@pytest.mark.parametrize("design", T.DESIGNS)
def test_forms_score_designs(ops, form, design):
    """S1 (maximum rises in every tile), S3 (one-hot) and S4 (all scores tie) under the masked tail M3, whose keys would carry most of
    the probability; S2 (maximum falls in every tile) under the head mask, a masked tail being blind there."""
    c = PRIMARY[form]
    mname, build = T.design_mask(design, c[4])
    for mode in c[6]:
        q, k, v, mask, ref, B, S = reference(c, design, mname, build, mode)
        check(c, mode, f"{design} {mname}", launch(ops, c, mode, q, k, v, mask), ref, B, S)


LAYOUTS = [(f, l) for f in PRIMARY for l in ("L1", "L3")] + [("F1", "L2"), ("F3", "L2")]   # L2 cannot reach 4096 tiles at a small size


@pytest.mark.parametrize("form,layout", LAYOUTS)
def test_layouts(ops, form, layout):
    """L1: packed qk (ldq = ldk = 2E, K = Q + E).  L2: batch stride below the row stride for q, k, v and out.  L3: output columns
    inside a wider NaN-patterned buffer that must stay bit-identical around them.  Inputs unchanged bit for bit (launch)."""
    c = PRIMARY[form]
    for mode in c[6]:
        q, k, v, mask, ref, B, S = reference(c, "N", "M2", T.mask_m2, mode, share=True)
        check(c, mode, f"layout {layout}", launch(ops, c, mode, q, k, v, mask, layout), ref, B, S)


@pytest.mark.parametrize("form", list(PRIMARY))
def test_all_masked_batch_entry(ops, form):
    """M7: an entry with no kept key comes out as finite zeros (every form reads l > 0 ? 1 / l : 0; torch gives NaN); the other
    entries are inside the bound."""
    c = PRIMARY[form]
    for mode in c[6]:
        q, k, v, mask, ref, B, S = reference(c, "N", "M7", T.mask_m7, mode)
        out = launch(ops, c, mode, q, k, v, mask)
        assert bool((_bits(out[1]) & 0x7FFFFFFF == 0).all()), f"{c[0]} [{mode}]: the all-masked entry is not all zeros"
        check(c, mode, "N M7", out, ref, B, S)


@pytest.mark.parametrize("form", list(PRIMARY))
def test_nonfinite_k_at_masked_keys(ops, form):
    """"Ignore" holds whatever the key's K row contains: the K rows of the masked keys hold +Inf, NaN and 3e38 in turn (V stays
    finite there), and the result is the reference over the kept keys.  The kernels that add the mask sentinel to the score instead
    of selecting it turn such a key into a valid score of 0.  Polls the range flag itself and records whether it was raised."""
    c = PRIMARY[form]
    ops.check_range()
    for mode in c[6]:
        q, k, v, mask, ref, B, S = reference(c, "N", "M2", T.mask_m2, mode, share=True)
        k = k.clone()
        bad = torch.tensor([float("inf"), float("nan"), 3.0e38])
        bi, ji = torch.nonzero(mask, as_tuple=True)
        k[bi, ji] = bad[ji % 3][:, None]
        out = launch(ops, c, mode, q, k, v, mask)
        try:
            ops.check_range()
            raised = False
        except ops.RangeError:
            raised = True
        NOTES.append(f"{c[0]} [{mode}] non-finite K at masked keys: range flag {'raised' if raised else 'not raised'}")
        check(c, mode, "non-finite K at masked keys", out, ref, B, S)


@pytest.mark.parametrize("mode", T.SPLIT_MODES)
def test_form_agreement(ops, mode):
    """F3, F5 and F6 on the same kept keys: the dispatcher gives Lk >= 1024 below 4096 tiles to F5, so F3 runs the first 1023 keys of
    the buffers and F5 / F6 all 1024 with key 1023 masked.  Pairwise |a - b| <= 2 B, the bound of the shared reference."""
    c3, c5, c6 = BOUNDARY["F3 at Lk=1023"], BOUNDARY["F5 at Lk=1024"], BOUNDARY["F6 at Lk=1024"]
    _, batch, nh, Lq, _, _, _ = c5
    q, k, v = T.operands("N", batch, nh, Lq, 1024, seed=5)
    m3 = T.mask_m2(batch, 1023)
    m5 = torch.cat([m3, torch.ones(batch, 1, dtype=torch.uint8)], 1)
    ref, B, S = T.masked_ref_and_bound(q, k[:, :1023], v[:, :1023], m3, nh, product=T.PRODUCT[mode], device="cuda")
    outs = {"F3": launch(ops, c5, mode, q, k, v, m3, Lk=1023), "F5": launch(ops, c5, mode, q, k, v, m5), "F6": launch(ops, c6, mode, q, k, v, m5)}
    for f, o in outs.items():
        check((f,), mode, "agreement (1023 kept-key range)", o, ref, B, S)
    for a, b in (("F3", "F5"), ("F3", "F6"), ("F5", "F6")):
        d = (outs[a].double() - outs[b].double()).abs()
        r = float(torch.where(d == 0, torch.zeros_like(d), d / (2 * B)).nan_to_num(nan=float("inf")).max())
        print(f"{a} against {b} [{mode}]: |a - b| / 2B {r:.3g}")
        assert r <= 1.0, f"{a} against {b} [{mode}]: worst |a - b| / 2B = {r:.3g}"


def test_zz_write_profile(ops):
    """Writes the table of every case above (run the whole module: each test appends its lines)."""
    best = {}
    for form, mode, fam, rB, rS in RESULTS:
        o = best.get((form, mode, fam), (0.0, 0.0))
        best[(form, mode, fam)] = (max(o[0], rB), max(o[1], rS))
    ran = {(f, m) for f, m, _ in best}
    need = {(c[0], m) for c in T.PRIMARY for m in c[6]}
    assert need <= ran, f"forms that did not run: {sorted(need - ran)}"
    with open(PROFILE, "w") as f:
        f.write("# tests/test_attn_forms_gpu.py on an MI355X: per (launch form, arithmetic mode, mask / score / layout family), the largest\n"
                "# |out - fp64 ref over the kept keys| over the whole output as a fraction of the derived bound B (no margin) and of\n"
                "# S = sum_j p_j |v_j|.  Forms F1..F7: tests/_attn.py mha_form.\n"
                "# form | mode | family | max err/B | max err/S\n")
        for (form, mode, fam), (rB, rS) in sorted(best.items()):
            f.write(f"{form} | {mode} | {fam} | {rB:.3f} | {rS:.3e}\n")
        for n in NOTES:
            f.write(f"# {n}\n")
