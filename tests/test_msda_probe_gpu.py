"""GPU: every form of the multi-scale deformable attention forward (csrc/msda.hip) against the fp64 reference of tests/_msda.py, element
by element, under the bound B derived there (not calibrated on what the kernels return, no margin added).  The inputs are structural
probes in which a defect is the whole of an output: lattices that sit on every border of every level (and of the valid region of a
padded level), one-hot point probes over integer-coded value rows, logits of scale 1 / 30 / 100, and item counts that leave tails in
every workgroup shape.  tests/test_msda_probe_cpu.py shows that a correct fp32 evaluation is inside B on these inputs and that each
defect of _msda.MUTANTS is >= 4 x outside.

How a form is reached (the dispatch of tce_msda_fused_valid_f32 and tce_ms_deform_attn_forward_f32 is restated in fused_form /
plain_form below and asserted for every case): see FUSED and PLAIN.  Every case appends (form, case, max err / B, max err / max|ref|)
to a table the last test writes to profiles/r16_msda_probe_by_form.txt."""
import functools
import os

import pytest
import torch

import _msda as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r16_msda_probe_by_form.txt")
RESULTS = []


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
    ops.check_range()
    yield
    ops.check_range()   # no case may raise the range flag


def dev(t):
    return t.cuda().contiguous()


def off4(t):
    """The tensor at a 4-byte offset inside a larger allocation: contiguous, not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ---------------------------------------------------------------------------------------------------------------
def fused_form(c, lds, fewq, aligned):
    """tce_msda_fused_valid_f32: which kernel a call takes (g_msda_lds = lds, g_msda_fewq = fewq)."""
    N, Lq, M, L, P, shapes = c["N"], c["Lq"], c["M"], c["L"], c["P"], c["shapes"]
    S, total = K.n_rows(shapes), N * Lq * M
    fits30 = N * S * M * 32 < 2 ** 30
    if (M == 8 and Lq >= 2048 and lds == 1 and c["valid"] is None and L == 4 and P == 4 and fits30 and aligned
            and shapes[-1][0] * shapes[-1][1] * 128 <= 160 * 1024):
        return "msda_fused_lds_kernel"
    if fewq and aligned and total <= 8192:
        return "msda_fused_fewq_kernel"
    if aligned:
        if L == 4 and P == 4 and lds != 2 and fits30 and M & (M - 1) == 0 and S < 2 ** 24 and total < 2 ** 31:
            return "msda_fused_q4u_kernel<2>" if lds == 3 else "msda_fused_q4u_kernel<4>"
        return "msda_fused_q4_kernel"
    return "msda_fused_kernel"


def plain_form(c, aligned):
    """tce_ms_deform_attn_forward_f32."""
    D, LP = c["value"].shape[-1], c["L"] * c["P"]
    if D != 32 or LP > 32:
        return "msda_generic_dev_kernel"
    return "msda_plain_q4_dev_kernel" if LP <= 16 and aligned else "msda_plain_dev_kernel"


# form id -> (kernel, how it is reached).  Ms: head counts, one per lattice variant (cycled); big: more than 8192 items.
FUSED = {
    # total <= 8192, both switches at their defaults; the via-ref lattices have 4 x the queries and run at M = 4
    "fewq": dict(kernel="msda_fused_fewq_kernel", Ms=(8, 3, 4, 4), big=False),
    # total > 8192, L = P = 4, M a power of two
    "q4u4": dict(kernel="msda_fused_q4u_kernel<4>", Ms=(8, 4, 2, 8), big=True),
    # as above with set_lds(3)
    "q4u2": dict(kernel="msda_fused_q4u_kernel<2>", Ms=(8, 4, 2, 8), big=True, lds=3),
    # set_lds(2) turns q4u off
    "q4_lds2": dict(kernel="msda_fused_q4_kernel", Ms=(8, 2, 8, 4), big=True, lds=2),
    # M = 3 is no power of two: q4u is off by itself
    "q4_m3": dict(kernel="msda_fused_q4_kernel", Ms=(3,), big=True),
    # L * P < 16 takes the q4 loop and its have[] lanes; few queries, so set_fewq(0) keeps the call off the few-query form
    "q4_lp": dict(kernel="msda_fused_q4_kernel", Ms=(8, 3, 8, 4), big=False, fewq=0, LPs=((3, 4), (2, 2), (1, 1), (4, 3))),
    # value and out at a 4-byte offset: the dword fallback, whatever the item count
    "dword": dict(kernel="msda_fused_kernel", Ms=(8, 3, 8, 3), big=True, misalign=True),
    # set_lds(1), M = 8, Lq >= 2048, N = 1, un-padded
    "lds": dict(kernel="msda_fused_lds_kernel", Ms=(8,), big=False, lds=1, min_lq=2048, N=1, padded=False, dense=(1, 2051)),
    # tce_msda_fewq_raw_f32: N * Lq * 8 <= 65536 (one workgroup per item; the product calls it with a few queries per frame)
    "raw": dict(kernel="msda_fewq_raw_kernel", Ms=(8,), big=False, raw=True, limit=65536, max_n=1, dense=(3, 5)),
}
PLAIN = {
    # D = 32, L * P <= 16, aligned
    "plain_q4": dict(kernel="msda_plain_q4_dev_kernel", D=32, P=4, Ms=(8, 3)),
    # L * P = 32
    "plain_lp32": dict(kernel="msda_plain_dev_kernel", D=32, P=8, Ms=(8, 3)),
    # value at a 4-byte offset
    "plain_unaligned": dict(kernel="msda_plain_dev_kernel", D=32, P=4, Ms=(8, 3), misalign=True),
    # head dims other than 32, L * P = 64
    "generic_d2": dict(kernel="msda_generic_dev_kernel", D=2, P=16, Ms=(8, 3)),
    "generic_d30": dict(kernel="msda_generic_dev_kernel", D=30, P=16, Ms=(3,)),
    "generic_d71": dict(kernel="msda_generic_dev_kernel", D=71, P=16, Ms=(3,)),
}
LATTICE = ((K.SHAPES_ODD, "off", 2, 0), (K.SHAPES_POW2, "off", 4, 0), (K.SHAPES_POW2, "ref", 2, 1), (K.SHAPES_ODD, "ref", 4, 0))
PADDED = ((K.SHAPES_ODD, K.VALID_ODD, "off", 2, 0), (K.SHAPES_POW2, K.VALID_POW2, "ref", 2, 1), (K.SHAPES_POW2, K.VALID_POW2, "off", 4, 0))


def frames_and_reps(f, nq, M):
    """(N, reps) for a lattice of nq queries: past 8192 items for the 8-lane forms, at most 8192 otherwise, Lq >= min_lq."""
    reps = max(1, -(-f.get("min_lq", 1) // nq))
    if "N" in f:
        return f["N"], reps
    if f["big"]:
        return -(-8193 // (nq * reps * M)), reps
    N = min(f.get("max_n", 2), f.get("limit", 8192) // (nq * reps * M))
    assert N >= 1, "lattice too large for a few-query form at this head count"
    return N, reps


@functools.lru_cache(maxsize=None)
def lattice_case(shapes_id, valid_id, N, M, L, P, mode, rd, rpf, reps, raw):
    shapes = (K.SHAPES_ODD, K.SHAPES_POW2)[shapes_id]
    valid = None if valid_id is None else (K.VALID_ODD, K.VALID_POW2)[valid_id]
    c = K.lattice_fused(shapes, valid, N, M, L, P, mode, rd, rpf, 100 + shapes_id, reps=reps, raw=raw)
    return (c,) + K.ref_and_bound(c)


@functools.lru_cache(maxsize=None)
def dense_case(N, Lq, M, L, P, rd, rpf, scale, onehot, raw, padded):
    c = K.dense_fused(K.SHAPES_ODD, K.VALID_ODD if padded else None, N, Lq, M, L, P, rd, rpf, 200 + M, logit_scale=scale, onehot=onehot,
                      raw=raw, code=onehot and not raw)
    return (c,) + K.ref_and_bound(c)


@functools.lru_cache(maxsize=None)
def plain_case(kind, shapes_id, N, Lq, M, D, P, scale):
    shapes = (K.SHAPES_ODD, K.SHAPES_POW2)[shapes_id]
    if kind == "lattice":
        c = K.lattice_plain(shapes, N, M, D, P, 300 + shapes_id)
    else:
        c = K.dense_plain(shapes, N, Lq, M, D, P, 310 + M, logit_scale=scale, onehot=kind == "onehot", code=kind == "onehot")
    return (c,) + K.ref_and_bound(c)


def run_fused(ops, lib, f, c):
    """One call of the case through the form's switches; asserts that the restated dispatch selects the form's kernel."""
    lds, fewq, mis = f.get("lds", 0), f.get("fewq", 1), f.get("misalign", False)
    N, Lq, M, L, P, shapes = c["N"], c["Lq"], c["M"], c["L"], c["P"], c["shapes"]
    S = K.n_rows(shapes)
    if f.get("raw"):
        assert N * Lq * 8 <= 65536
        return ops.msda_fewq_raw(dev(c["src"]), dev(c["wv"]), dev(c["bv"]), dev(c["proj"]), dev(c["ref"]), shapes, N, S, Lq, L, P,
                                 c["ref_dim"], bool(c["ref_per_frame"]), valid_hw=c["valid"])
    assert fused_form(c, lds, fewq, not mis) == f["kernel"], (fused_form(c, lds, fewq, not mis), f["kernel"])
    value = off4(c["value"]) if mis else dev(c["value"])
    out = off4(torch.zeros(N * Lq, M * 32)) if mis else None
    lib.tce_debug_msda_set_lds(lds)
    lib.tce_debug_msda_set_fewq(fewq)
    try:
        out = ops.msda_fused(value, dev(c["proj"]), dev(c["ref"]), shapes, N, S, M, Lq, L, P, c["ref_dim"], bool(c["ref_per_frame"]),
                             out=out, valid_hw=c["valid"])
        torch.cuda.synchronize()
    finally:
        lib.tce_debug_msda_set_lds(0)
        lib.tce_debug_msda_set_fewq(1)
    return out


def run_plain(ops, f, c):
    mis = f.get("misalign", False)
    assert plain_form(c, not mis) == f["kernel"]
    shapes = c["shapes"]
    sh = torch.tensor(shapes, dtype=torch.int64)
    lsi = torch.cat([sh.new_zeros(1), (sh[:, 0] * sh[:, 1]).cumsum(0)[:-1]])
    value = off4(c["value"]) if mis else dev(c["value"])
    return ops.ms_deform_attn_forward(value, sh.cuda(), lsi.cuda(), dev(c["loc"]), dev(c["weights"]))


def check(form, c, ref, B, out):
    """Per-element |out - ref| <= B; records the case."""
    r, i, rel = K.worst(out, ref, B)
    name = f"{c['note']}, {'x'.join(f'{h}.{w}' for h, w in c['shapes'])}, N {c['N']} Lq {c['Lq']} M {c['M']} L {c['L']} P {c['P']}"
    if c["kind"] != "plain":
        name += f", ref_dim {c['ref_dim']}{' per frame' if c['ref_per_frame'] else ''}{', padded' if c['valid'] is not None else ''}"
    else:
        name += f", D {c['value'].shape[-1]}"
    print(f"{form} | {name} | err/B {r:.3f} | err/max|ref| {rel:.2e}")
    RESULTS.append((form, name, r, rel))
    if not r <= 1.0:
        o, rf = out.detach().cpu().double().flatten()[i], ref.flatten()[i]
        n_bad = int(((out.detach().cpu().double().reshape(ref.shape) - ref).abs() > B).sum())
        msg = (f"{form} [{name}]: {n_bad} of {ref.numel()} elements outside the bound; worst err/B = {r:.3g} (out {float(o):.9g}, "
               f"ref {float(rf):.9g}) at {K.describe(c, i)}")
        if c["note"] == "one-hot" and c.get("value") is not None:
            D = c["value"].shape[-1]
            msg += f"; row code, head, channel read: {K.decode(o, c['M'], D)}, expected: {K.decode(rf, c['M'], D)}"
        raise AssertionError(msg)


def _lp(f, i):
    return f["LPs"][i % len(f["LPs"])] if "LPs" in f else (4, 4)


# ---------------------------------------------------------------------------------------------------------------
# fused forms and the sample-then-project form
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", range(len(LATTICE)))
@pytest.mark.parametrize("form", list(FUSED))
def test_fused_border_lattice(ops, lib, form, variant):
    f = FUSED[form]
    shapes, mode, rd, rpf = LATTICE[variant]
    M = f["Ms"][variant % len(f["Ms"])]
    L, P = _lp(f, variant)
    N, reps = frames_and_reps(f, 289 * (L if mode == "ref" else 1), M)
    c, ref, B = lattice_case(int(shapes is K.SHAPES_POW2), None, N, M, L, P, mode, rd, rpf, reps, bool(f.get("raw")))
    check(f["kernel"], c, ref, B, run_fused(ops, lib, f, c))


@pytest.mark.parametrize("variant", range(len(PADDED)))
@pytest.mark.parametrize("form", [k for k, f in FUSED.items() if f.get("padded", True)])
def test_fused_padded_border_lattice(ops, lib, form, variant):
    """Every form that takes valid_hw (the LDS form rejects it by dispatch)."""
    f = FUSED[form]
    shapes, valid, mode, rd, rpf = PADDED[variant]
    M = f["Ms"][variant % len(f["Ms"])]
    L, P = _lp(f, variant)
    N, reps = frames_and_reps(f, 441 * (L if mode == "ref" else 1), M)
    sid = int(shapes is K.SHAPES_POW2)
    c, ref, B = lattice_case(sid, sid, N, M, L, P, mode, rd, rpf, reps, bool(f.get("raw")))
    check(f["kernel"], c, ref, B, run_fused(ops, lib, f, c))


def dense_sizes(f, M):
    """(N, Lq): N * Lq odd (no multiple of 8 or 32), so N * Lq * M is no multiple of 4 / 8 / 32 unless M itself is."""
    if "dense" in f:
        return f["dense"]
    if f["big"]:
        return 3, {8: 347, 4: 685, 3: 929, 2: 1367}[M]     # 8328, 8220, 8361, 8202 items
    return 3, 37                                            # 111 (frame, query) pairs


@pytest.mark.parametrize("form", list(FUSED))
def test_fused_one_hot_points(ops, lib, form):
    """Every point slot that exists, in turn, is the only one with weight (slot (q + m + 3 n) % (L * P)); the value rows are integer
    codes of (row rotated per frame, head, channel)."""
    f = FUSED[form]
    for i, M in enumerate(dict.fromkeys(f["Ms"])):
        for j, (L, P) in enumerate(f.get("LPs", ((4, 4),))):
            N, Lq = dense_sizes(f, M)
            rd = 2 if (i + j) % 2 == 0 else 4
            c, ref, B = dense_case(N, Lq, M, L, P, rd, 1, 1.0, True, bool(f.get("raw")), f.get("padded", True) and (i + j) % 2 == 1)
            check(f["kernel"], c, ref, B, run_fused(ops, lib, f, c))


@pytest.mark.parametrize("scale", K.LOGIT_SCALES)
@pytest.mark.parametrize("form", list(FUSED))
def test_fused_logit_range_and_tails(ops, lib, form, scale):
    """The same dense case at logit scales 1, 30 and 100 (at 100 an exponent taken without the row maximum overflows), at item counts
    that leave a tail in every workgroup shape."""
    f = FUSED[form]
    for i, M in enumerate(dict.fromkeys(f["Ms"])):
        L, P = _lp(f, i)
        N, Lq = dense_sizes(f, M)
        c, ref, B = dense_case(N, Lq, M, L, P, 4 if i % 2 else 2, i % 2, scale, False, bool(f.get("raw")), False)
        check(f["kernel"], c, ref, B, run_fused(ops, lib, f, c))


# ---------------------------------------------------------------------------------------------------------------
# the reference-signature op
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(PLAIN))
def test_plain_border_lattice(ops, form):
    f = PLAIN[form]
    for sid, M in zip((0, 1), (f["Ms"] * 2)[:2]):
        c, ref, B = plain_case("lattice", sid, 2, 0, M, f["D"], f["P"], 1.0)
        check(f["kernel"], c, ref, B, run_plain(ops, f, c))


@pytest.mark.parametrize("form", list(PLAIN))
def test_plain_one_hot_points(ops, form):
    f = PLAIN[form]
    for M in f["Ms"]:
        c, ref, B = plain_case("onehot", 0, 3, 4 * f["P"] + 5, M, f["D"], f["P"], 1.0)
        check(f["kernel"], c, ref, B, run_plain(ops, f, c))


@pytest.mark.parametrize("scale", K.LOGIT_SCALES)
@pytest.mark.parametrize("form", list(PLAIN))
def test_plain_logit_range_and_tails(ops, form, scale):
    """The plain op takes weights: it gets the fp32 softmax of the scaled logits.  3 x 37 x M items: a tail in every workgroup shape."""
    f = PLAIN[form]
    for M in f["Ms"]:
        c, ref, B = plain_case("dense", 0, 3, 37, M, f["D"], f["P"], scale)
        check(f["kernel"], c, ref, B, run_plain(ops, f, c))


# ---------------------------------------------------------------------------------------------------------------
# bit identity of the 16-byte forms
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True])
def test_sixteen_byte_forms_are_bit_identical_on_the_lattice(ops, lib, padded):
    """The claims of test_msda_fused_lds_staged_is_bit_identical (default = four points in flight, the LDS-staged form, the one-by-one
    loop, two in flight) where they are hardest: on the borders.  The branch-free forms multiply an absent corner by a zero coefficient
    where the loop adds nothing, which can change the sign of a zero and nothing else: + 0.0 maps -0.0 to 0.0.  (Padded, mode 1 is
    rejected by the dispatch and the call takes the default form.)"""
    nq = 441 if padded else 289
    c, ref, B = lattice_case(0, 0 if padded else None, 1, 8, 4, 4, "off", 2, 0, -(-2048 // nq), False)
    outs = {}
    for mode in (0, 1, 2, 3):
        f = dict(lds=mode, kernel=fused_form(c, mode, 1, True))
        outs[mode] = run_fused(ops, lib, f, c) + 0.0
    assert fused_form(c, 1, 1, True) == ("msda_fused_q4u_kernel<4>" if padded else "msda_fused_lds_kernel")
    for mode in (1, 2, 3):
        assert torch.equal(outs[0], outs[mode]), f"mode {mode} differs from the default form in {int((outs[0] != outs[mode]).sum())} elements"


# ---------------------------------------------------------------------------------------------------------------
# byte offsets past 2^31
# ---------------------------------------------------------------------------------------------------------------
BIG_SHAPES = [(360, 640), (180, 320), (90, 160), (45, 80)]     # S = 306 000 rows of 1 KiB at M = 8


def big_value_fn(i):
    """An integer in [0, 240] from the flat element index (int64).  Rows 241 k apart repeat; a slip of 2^31 or 2^32 bytes is 2^21 or
    2^22 rows = 211 or 181 (mod 241), so it lands on other values."""
    return ((i * 48271) % 241).float()


@pytest.mark.parametrize("N,Lq,kernel", [(13, 128, "msda_fused_q4u_kernel<4>"), (13, 8, "msda_fused_fewq_kernel"),
                                         (14, 128, "msda_fused_q4_kernel")])
def test_large_value_tensor_offsets(ops, lib, N, Lq, kernel):
    """A supported size: N = 13 is N*S*M*D = 1 018 368 000 < 2^30 elements, a 4.07 GB tensor whose byte offsets pass 2^31 from frame 7
    on -- legal for the 32-bit offsets of msda_fused_q4u_kernel (lane_off + (start << 10) + (idx << 10) < N*S*1024 < 2^32, unsigned
    throughout) and for the 64-bit ones of the few-query form; N = 14 crosses 2^30 and the launcher must fall to the loop form.  One-hot
    probes; frame 0 aims at the first rows of the tensor and the last frame at its last rows.  value is filled on the device from
    big_value_fn and the reference evaluates the same formula at the rows it gathers."""
    S, M = K.n_rows(BIG_SHAPES), 8
    c = K.dense_fused(BIG_SHAPES, None, N, Lq, M, 4, 4, 2, 1, 400 + N + Lq, onehot=True, value=False, edges=True)
    assert fused_form(c, 0, 1, True) == kernel
    ref, B = K.ref_and_bound_fn(c, big_value_fn, 240.0)
    value = torch.empty(N, S * M * 32, dtype=torch.float32, device="cuda")
    per = S * M * 32
    for n in range(N):
        value[n] = big_value_fn(torch.arange(n * per, (n + 1) * per, dtype=torch.int64, device="cuda"))
    out = ops.msda_fused(value, dev(c["proj"]), dev(c["ref"]), BIG_SHAPES, N, S, M, Lq, 4, 4, 2, True)
    torch.cuda.synchronize()
    del value
    check(kernel, c, ref, B, out)


# ---------------------------------------------------------------------------------------------------------------
def test_zz_write_profile(ops):
    """Writes the table of every case above (run the whole module: each test appends its lines)."""
    need = {f["kernel"] for f in FUSED.values()} | {f["kernel"] for f in PLAIN.values()}
    seen = {r[0] for r in RESULTS}
    assert need <= seen, f"forms that did not run: {sorted(need - seen)}"
    worst = {}
    for form, name, r, rel in RESULTS:
        w = worst.setdefault(form, [0.0, 0.0, 0])
        w[0], w[1], w[2] = max(w[0], r), max(w[1], rel), w[2] + 1
    with open(PROFILE, "w") as fh:
        fh.write("# tests/test_msda_probe_gpu.py on an MI355X: per form the worst case, then per case, the largest |out - fp64 ref| over the\n"
                 "# output as a fraction of the derived bound B (tests/_msda.py) and of max|ref|.\n"
                 "# form | cases | worst err/B | worst err/max|ref|\n")
        for form in sorted(worst):
            fh.write(f"{form} | {worst[form][2]} | {worst[form][0]:.3f} | {worst[form][1]:.2e}\n")
        fh.write("# form | case | err/B | err/max|ref|\n")
        for form, name, r, rel in sorted(set(RESULTS)):
            fh.write(f"{form} | {name} | {r:.3f} | {rel:.2e}\n")
    assert all(w[0] <= 1.0 for w in worst.values())
