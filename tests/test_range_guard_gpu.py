"""GPU: every store site of the split-fp16 arithmetic is held to the range guard (include/tce_rvos.h, tce_set_range_flag).

Per site and launch form of tests/_range.py SITES: one launch and one ops.check_range() per (target, value class, route) -- the flag is
a single bit, so every position needs its own launch -- in mode "f16x3" and again in mode "f16" (weights re-packed in the mode).  The
expectation comes from _range.expected_flag on the case's fp64 reference; the case's inputs satisfy _range.check_condition.  A case
with an Inf / NaN also reads the output back: only the rows the reference marks may hold non-finite values (the zero-fill of pad
rows must not spread a NaN).  Then: mode "f32" pinned (no contract, no flag), false positives (every output in +-[50000, 59000] on
a ragged last tile; NaN just past every operand's extent), the asynchronous half (range_snapshot_async / range_poll), stickiness,
and a captured launch replayed over a clean and then an offending input.

The last test writes one line per (site, form, shape) to profiles/r25_range_guard.txt; a line keeps the result recorded for the
parent commit (the run before the fixes: TCE_RANGE_RECORD_AS=parent) beside this build's."""
import ctypes as C
import os

import pytest
import torch

import _range as R
from _footprint import Slab

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r25_range_guard.txt")
MODES = ("f16x3", "f16")
RESULTS = {}
QNAN = 0x7FC00000


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tce_rvos_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from tce_rvos_amd._lib import lib as _lib
    return _lib()


def raised(ops):
    """One ops.check_range(): True when the flag was up (the raise clears it)."""
    try:
        ops.check_range()
    except ops.RangeError:
        return True
    return False


@pytest.fixture(autouse=True)
def _flag_starts_and_ends_clean(ops):
    raised(ops)
    yield
    raised(ops)


def dev(name, t):
    return None if t is None else t.cuda().contiguous()


def run_case(ops, lib, case, mode, put=dev):
    """Launches the case in `mode`; returns the list of what went wrong (empty = the guard did what the reference says)."""
    with ops.arith(mode):
        out = case.launch(ops, lib, put)
    flag = raised(ops)
    wrong = []
    if flag != case.expect:
        wrong.append(f"{case.label} mode {mode}: flag {'raised' if flag else 'clean'}, reference says {'raise' if case.expect else 'clean'}")
    fin = torch.isfinite(out)
    if case.cls in ("inf", "nan"):
        bad_rows = set(torch.nonzero(~fin.all(1)).flatten().tolist())
        if not bad_rows <= set(case.nan_rows):
            wrong.append(f"{case.label} mode {mode}: non-finite values in rows {sorted(bad_rows - set(case.nan_rows))[:8]} that must be clean")
    elif not bool(fin.all()):
        wrong.append(f"{case.label} mode {mode}: non-finite output in a finite case")
    return wrong


@pytest.mark.parametrize("site", R.SITES, ids=[s.id for s in R.SITES])
def test_store_site_reports(ops, lib, site):
    wrong, n, classes, vias = [], 0, [], []
    try:
        for case in site.cases():
            R.check_condition(case)
            n += 1
            classes.append(case.cls)
            vias.append(case.via)
            for mode in site.modes:
                wrong += run_case(ops, lib, case, mode)
    finally:
        missed = sorted({w.split(" target ")[1].split(" mode ")[0] for w in wrong if " target " in w})
        RESULTS[site.id] = (site, n, sorted(set(classes), key=R.ALL.index), sorted(set(vias)), len(wrong), missed)
    assert not wrong, f"{len(wrong)} of {n * len(site.modes)} launches:\n" + "\n".join(wrong[:12])


def test_mode_f32_has_no_contract(ops, lib):
    """The same over-limit GEMM in exact fp32 leaves the flag clean: the tiled kernel, the fix-up pass and the split-K reduce."""
    a, w, bias, res, ref = R.linear_operands(130, 72, 64, 77, 40, "over+", "res_add", R.ACT_GELU, R.RES_ADD, 1)
    assert R.expected_flag(ref.numpy())
    with ops.arith("f32"):
        ops.gemm(dev("a", a), dev("w", w), bias=dev("b", bias))
        ops.gemm(dev("a", a), dev("w", w), bias=dev("b", bias), act=R.ACT_GELU, res=dev("r", res), res_mode=R.RES_ADD)
        a2, w2, b2, _, ref2 = R.linear_operands(25, 256, 2048, 7, 40, "over+", "sum", seed=3)
        assert R.expected_flag(ref2.numpy())
        ops.gemm_ex(dev("a", a2), dev("w", w2), torch.zeros(25, 256, device="cuda"), 25, 256, 2048, 2048, 2048, 256, bias=dev("b", b2),
                    splitk=8, ws=torch.zeros(8 * 25 * 256, device="cuda"))
    assert not raised(ops)
    ops.gemm(dev("a", a), dev("w", w), bias=dev("b", bias), act=R.ACT_GELU, res=dev("r", res), res_mode=R.RES_ADD)
    assert raised(ops)   # the very same launch in the default split mode


def test_partial_plane_alone_is_conservative(ops):
    """Documented behaviour, recorded and not changed: a partial plane over the limit raises the flag although the summed result
    (60160 - 59904 = 256) is in range -- the partial launch reports on what IT stores."""
    a, w, bias, _, _ = R.linear_operands(25, 256, 2048, 7, 40, "clean", "sum", seed=3)
    a[7, 3], a[7, 2048 - 5], w[40, 3], w[40, 2048 - 5], bias[40] = 256.0, 256.0, 235.0, -234.0, 0.0
    ref = a.double() @ w.double().T + bias.double()
    assert not R.expected_flag(ref.numpy()) and float(ref[7, 40]) == 256.0 + 0.0
    out = ops.gemm_ex(dev("a", a), dev("w", w), torch.zeros(25, 256, device="cuda"), 25, 256, 2048, 2048, 2048, 256, bias=dev("b", bias),
                      splitk=8, ws=torch.zeros(8 * 25 * 256, device="cuda"))
    assert raised(ops)
    assert float(out[7, 40]) == 256.0


# ---------------------------------------------------------------------------------------------------------------------
# false positives
# ---------------------------------------------------------------------------------------------------------------------
def _near_launches(ops, lib):
    """(family, fn(a, w, put) -> out) with ragged last tiles; every output of near_operands lies within +-[50000, 59000]."""
    def gemm(M, N, K):
        return lambda a, w, put: ops.gemm(put("a", a), put("w", w), out=put("out", torch.zeros(M, N)))

    def rowlin(M, N, K):
        return lambda a, w, put: ops.rowlin(put("a", a), ops.rowlin_pack(put("w", w)), put("out", torch.zeros(M, N)), M, N, K, K, N)

    def splitk(M, N, K, s):
        return lambda a, w, put: ops.gemm_ex(put("a", a), put("w", w), put("out", torch.zeros(M, N)), M, N, K, K, K, N, splitk=s,
                                             ws=put("ws", torch.zeros(s * M * N)))

    def thin(M, N, K):
        s = K // 256
        return lambda a, w, put: ops.splitk_reduce(ops.thin_partials(put("a", a), put("w", w), put("ws", torch.zeros(s, M, N)), M, N, K),
                                                   s, M, N, put("out", torch.zeros(M, N)))
    return [("gemm tile 6464", 130, 72, 64, gemm(130, 72, 64)), ("gemm tile 6464, N % 4 != 0", 130, 70, 64, gemm(130, 70, 64)),
            ("gemm tile 12864", 6100, 512, 32, gemm(6100, 512, 32)), ("gemm tile 256128", 49100, 256, 32, gemm(49100, 256, 32)),
            ("rowlin", 129, 32, 96, rowlin(129, 32, 96)), ("rowlin", 200, 256, 384, rowlin(200, 256, 384)),
            ("split-K", 25, 256, 2048, splitk(25, 256, 2048, 8)), ("thin stream", 7, 768, 768, thin(7, 768, 768))]


def test_no_false_positive_near_the_limit(ops, lib):
    """Every valid output within +-[50000, 59000], M ragged in the last tile: pad rows and pad columns must not raise the flag."""
    wrong = []
    for name, M, N, K, fn in _near_launches(ops, lib):
        a, w, ref = R.near_operands(M, N, K)
        assert 50000 <= float(ref.abs().min()) and float(ref.abs().max()) <= 59000 and not R.expected_flag(ref.numpy())
        for mode in MODES:
            with ops.arith(mode):
                fn(a, w, dev)
            if raised(ops):
                wrong.append(f"{name} {M}x{N}x{K} mode {mode}")
    assert not wrong, wrong


def test_no_false_positive_near_the_limit_conv3x3_and_ffn(ops, lib):
    """The same for the two families whose operands are not a plain (a, w) pair.  3x3 convolution: channel k0 of every pixel is 256 and
    only the centre tap has a weight there (+-200 .. 230), so every output is that product plus an O(1) remainder.  Fused FFN: W1 = 0,
    so every output is the residual x (+-50000 .. 59000 itself) plus the constant W2 relu(b1) + b2 of O(1)."""
    import _arith
    T, H, W, Cin = 3, 17, 5, 256
    M = T * H * W
    x, wc, _ = R.near_operands(M, 256, Cin, seed=10)
    w = torch.zeros(256, 9, Cin)
    w[:, 4] = wc
    g = torch.Generator().manual_seed(3)
    rest = (torch.randn(256, 9, Cin, generator=g) / 48).half().float()
    rest[:, :, 3] = 0                      # column k0 = 3 of near_operands: no other tap sees the 256
    rest[:, 4] = 0
    w = (w + rest).reshape(256, 9 * Cin)
    ref = _arith.im2col(x, T, H, W, Cin, 3, 1, 1).double() @ w.double().T
    assert 50000 <= float(ref.abs().min()) and float(ref.abs().max()) <= 59000
    wrong = []
    for mode in MODES:
        with ops.arith(mode):
            ops.conv3x3(dev("x", x), ops.conv3x3_pack(dev("w", w), Cin), T, H, W, Cin, 256)
        if raised(ops):
            wrong.append(f"conv3x3 mode {mode}")
    Mf, C, Hd = 333, 256, 64
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    xf = sign[None, :] * (50100.0 + 8800.0 * torch.rand(Mf, C, generator=g)).half().float()
    b1, w2, b2 = torch.rand(Hd, generator=g), (torch.randn(C, Hd, generator=g) / 8).half().float(), torch.randn(C, generator=g) * 0.2
    ref = xf.double() + (w2.double() @ b1.double() + b2.double())[None, :]
    assert 50000 <= float(ref.abs().min()) and float(ref.abs().max()) <= 59000
    for mode in MODES:
        with ops.arith(mode):
            pk = ops.ffn_pack(dev("w1", torch.zeros(Hd, C)), dev("b1", b1), dev("w2", w2))
            ops.ffn_fused(dev("x", xf), pk, dev("b2", b2), Hd, R.ACT_RELU, out=torch.zeros(Mf, C, device="cuda"))
        if raised(ops):
            wrong.append(f"ffn mode {mode}")
    assert not wrong, wrong


SLAB_SITES =[s for s in R.SITES if s.shape in ("130x72x64", "130x70x64", "25x256x2048 / 8", "40x1024x512 / 2", "7x768x768", "32x768x768 -> 64",
                                                 "129x32x96", "200x256x384", "333x256x64", "300x96x384", "1x9x13 256->256", "3x17x5 256->256",
                                                 "1x7x7 C=128 shift=3", "1x30x41 -> 128", "1x9x7 64->96 3x3", "1x9x7 64->96 3x3 / 3",
                                                 "130 rows, 8 keys", "301 rows, 11 keys")
              and any("clean" in classes for _, classes in s.variants)]


@pytest.mark.parametrize("site", SLAB_SITES, ids=[s.id for s in SLAB_SITES])
def test_no_false_positive_from_nan_past_the_extents(ops, lib, site):
    """The clean case with every operand in a slab (tests/_footprint.py) whose guard bytes, just past each operand's extent, hold NaN:
    a kernel that lets a load past the extent reach its running maximum raises the flag here."""
    case = next(c for c in site.cases() if c.cls == "clean")
    R.check_condition(case)
    slab = Slab(96 << 20, device="cuda")
    for mode in site.modes:
        slab.begin(QNAN)
        n = [0]

        def put(name, t):
            if t is None:
                return None
            n[0] += 1
            if t.dim() > 2:   # slab buffers are row-pitched: anything deeper goes in as one dense run
                return slab.put(f"{name}{n[0]}", t.contiguous().reshape(-1)).view(t.shape)
            return slab.put(f"{name}{n[0]}", t.contiguous())
        assert run_case(ops, lib, case, mode, put) == []


# ---------------------------------------------------------------------------------------------------------------------
# the asynchronous half, stickiness, a captured launch
# ---------------------------------------------------------------------------------------------------------------------
def _gemm_pair():
    clean = R.linear_operands(130, 72, 64, 77, 40, "clean", "product", seed=1)
    bad = R.linear_operands(130, 72, 64, 77, 40, "over+", "product", seed=1)
    assert not R.expected_flag(clean[4].numpy()) and R.expected_flag(bad[4].numpy())
    return clean, bad


def test_async_snapshot_and_poll(ops):
    clean, bad = _gemm_pair()
    st = ops.range_flag()
    st["event"] = None
    ops.range_poll()                      # no snapshot pending: a no-op
    ops.range_poll(wait=True)
    ops.gemm(dev("a", bad[0]), dev("w", bad[1]), bias=dev("b", bad[2]))
    ops.range_snapshot_async()
    with pytest.raises(ops.RangeError):
        ops.range_poll(wait=True)
    ops.range_poll(wait=True)             # the raise consumed the snapshot and cleared the flag
    ops.range_snapshot_async()
    ops.range_poll(wait=True)
    assert int(st["flag"].item()) == 0


def test_flag_is_sticky_until_polled(ops):
    clean, bad = _gemm_pair()
    ops.gemm(dev("a", bad[0]), dev("w", bad[1]), bias=dev("b", bad[2]))
    for _ in range(3):                    # clean launches behind the offending one do not lower it
        ops.gemm(dev("a", clean[0]), dev("w", clean[1]), bias=dev("b", clean[2]))
    torch.cuda.synchronize()
    assert int(ops.range_flag()["flag"].item()) == 1
    ops.range_snapshot_async()
    with pytest.raises(ops.RangeError):
        ops.range_poll(wait=True)
    assert not raised(ops)


def test_captured_launch_reports_on_replay(ops, lib):
    """One GEMM launch captured on one stream (tce_graph_begin / tce_graph_end), replayed twice over the same input buffer: clean
    operands first (no flag), then the offending ones written into the same buffers (flag)."""
    clean, bad = _gemm_pair()
    a, w, b, out = dev("a", clean[0]), dev("w", clean[1]), dev("b", clean[2]), torch.zeros(130, 72, device="cuda")
    ops.range_flag()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ex = C.c_void_p()
    with torch.cuda.stream(side):
        assert lib.tce_graph_begin(side.cuda_stream) == 0
        ops.gemm(a, w, bias=b, out=out)
        assert lib.tce_graph_end(side.cuda_stream, C.byref(ex)) == 0
    try:
        assert not raised(ops)            # capturing launched nothing
        with torch.cuda.stream(side):
            assert lib.tce_graph_launch(ex, side.cuda_stream) == 0
        side.synchronize()
        assert not raised(ops)
        assert torch.equal(out.cpu().double(), clean[4]) or float((out.cpu().double() - clean[4]).abs().max()) < 1e-3
        a.copy_(bad[0])
        w.copy_(bad[1])
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert lib.tce_graph_launch(ex, side.cuda_stream) == 0
        side.synchronize()
        assert raised(ops)
        assert float(out[77, 40]) == 60160.0
    finally:
        lib.tce_graph_destroy(ex)


# ---------------------------------------------------------------------------------------------------------------------
def _parse(path):
    old = {}
    if os.path.exists(path):
        for line in open(path):
            if line.startswith("#") or " | " not in line:
                continue
            f = [x.strip() for x in line.rstrip("\n").split(" | ")]
            if len(f) >= 8:
                old[(f[0], f[1], f[2])] = (f[6], f[7])
    return old


def test_zz_write_profile():
    """One line per (site, form, shape); run the whole module.  The column this run fills is "this build", or "parent commit" when
    TCE_RANGE_RECORD_AS=parent (the run of this file against the library built from the parent commit)."""
    assert len(RESULTS) == len(R.SITES), f"sites that did not run: {sorted(set(s.id for s in R.SITES) - set(RESULTS))}"
    as_parent = os.environ.get("TCE_RANGE_RECORD_AS") == "parent"
    old = _parse(PROFILE)
    head = [line for line in (open(PROFILE) if os.path.exists(PROFILE) else []) if line.startswith("#")]
    if not head:
        head = ["# tests/test_range_guard_gpu.py on an MI355X: per store site and launch form, the targets (row, column) and value classes tried\n",
                "# (each in modes f16x3 and f16 where the form exists in both), and whether the range flag did what the fp64 reference says -- on the parent commit\n",
                "# (before the reports were added to the split-K reduces, the fix-up pass and the thin stream) and on this build.\n",
                "# entry [form] | source | shape | stored value | targets | classes (routes) | parent commit | this build\n"]
    with open(PROFILE, "w") as f:
        f.writelines(head)
        for sid in [s.id for s in R.SITES]:
            site, n, classes, vias, n_wrong, missed = RESULTS[sid]
            res = "ok" if not n_wrong else f"{n_wrong} of {len(site.modes) * n} launches wrong: " + "; ".join(missed[:4]) + (" ..." if len(missed) > 4 else "")
            key = (f"{site.entry} [{site.form}]", site.source, site.shape)
            parent, this = old.get(key, ("not run", "not run"))
            parent, this = (res, this) if as_parent else (parent, res)
            tg = " ".join(f"({r},{c})" for r, c in site.targets[:6]) + (f" +{len(site.targets) - 6}" if len(site.targets) > 6 else "")
            f.write(" | ".join([key[0], key[1], key[2], site.kind, tg, ", ".join(classes) + " (" + ", ".join(vias) + ")", parent, this]) + "\n")
