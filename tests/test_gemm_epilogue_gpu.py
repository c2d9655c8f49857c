"""GPU: the prologue and every epilogue form of tce_gemm_f32 / tce_gemm_splitk_f32 / tce_splitk_reduce_f32 against the references of
tests/_epilogue.py.  The product is EXACT on the exact-product design (see _epilogue.py), so what is compared is the wrapper alone:
bit equality with the fp32 chain of gemm_epilogue.h wherever there is no GELU / LayerNorm, and the evaluation bounds of _arith.py
(no product term) where there is.  A few dense cases compose the whole wrapper to first order as test_rowlin_tails does.

Every case stores into a NaN-filled wider buffer and everything around the outputs must still be NaN afterwards; bias and residual
lie in NaN-filled buffers too, so a read one element off poisons the output.  The tiles the launcher only picks at large shapes are
reached through tce_gemm_force_tile / tce_debug_set_epilogue; both, and the arithmetic mode, are restored after every case.

CASES is the table of every launch; tests/test_gemm_epilogue_cpu.py reads it (designs exact, planted defects caught).  The last test
writes one line per case to profiles/r29_gemm_epilogue_forms.txt."""
import ctypes as C
import os
from contextlib import contextmanager

import pytest
import torch

import _epilogue as E
from _epilogue import Case, conv_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r29_gemm_epilogue_forms.txt")
RESULTS = []
NAN = float("nan")

SPLIT_INSTANCES = [(mode, tile, epi) for mode in ("f16x3", "f16")
                   for tile, epi in ((6464, 1), (6465, 1), (12864, 1), (128128, 1), (256128, 1), (256128, 0))]
F32_INSTANCES = [("f32", tile, 1) for tile in (6464, 12864, 128128)]
EIGHT = E.FUSED + ((2, 1),)   # the seven fused combinations and one folded onto epi_fix_kernel


def pitch4(n):
    return (n + 3) // 4 * 4


def _instance_cases():
    """Every kernel instance, with and without the addend: M = BM + 35 (a full tile and a ragged one that ends inside a 32-row
    fragment) over every N (N in {29, 31, 33, 61} also with 4-float pitches: vector and scalar lanes in one wave), K = 32 / 96 / 160
    (1, 3, 5 slices against a ring of 4; K = 64 is the N sweep's), and M = 1.  The eight combinations rotate over the shapes."""
    for ii, (mode, tile, epi) in enumerate(SPLIT_INSTANCES + F32_INSTANCES):
        BM, BN = E.TILE_BM[tile], E.TILE_BN[tile]
        for a2 in (False, True):
            M = BM + 35
            shapes = [(M, N, N, 64) for N in (1, 3, 4, 28, 29, 31, 32, 33, 61, BN + 28, BN + 29, BN + 33)]
            shapes += [(M, N, pitch4(N), 64) for N in (29, 31, 33, 61)]
            shapes += [(M, BN + 29, pitch4(BN + 29), K) for K in (32, 96, 160)]
            shapes += [(1, 33, 36, 64), (1, BN + 28, BN + 28, 32)]
            for j, (M_, N, ld, K) in enumerate(shapes):
                act, res = EIGHT[(j + 3 * ii + 5 * a2) % 8]
                yield Case("instance", mode, tile, epi, M_, N, K, a2, act, res, ldc=ld, ldres=ld)


def _combo_cases():
    """All twelve combinations on the 6464 and 256128 tiles; the fused ones with a residual also in place (act 3 / res 1 in place is
    the ResNet bottleneck's launch)."""
    for mode, tile, epi in (("f16x3", 6464, 1), ("f32", 6464, 1), ("f16x3", 256128, 1), ("f16x3", 256128, 0), ("f16", 256128, 1)):
        M, N = E.TILE_BM[tile] + 35, E.TILE_BN[tile] + 29
        base = Case("combo", mode, tile, epi, M, N, 64, True, ldc=pitch4(N), ldres=pitch4(N))
        for act, res in E.COMBOS:
            yield E.replace(base, act=act, res_mode=res)
            if res and (act, res) in E.FUSED:
                yield E.replace(base, act=act, res_mode=res, inplace=True)


def _ring_cases():
    """The 64x64 tile's 1-slice ring is taken at >= 512 workgroups (gemm_f16x3_small.hip:15-17): 128 problems of 67 x 70 x 32."""
    for mode in ("f16x3", "f16"):
        for a2 in (False, True):
            yield Case("ring", mode, 6464, 1, 67, 70, 32, a2, 1, 1, batch=128)
            yield Case("ring", mode, 6464, 1, 67, 70, 32, a2, 0, 2, batch=128, ldc=72, ldres=72)


ALIGN_VARIANTS = (dict(), dict(c_off=1), dict(b_off=1), dict(r_off=1), dict(ldc=97), dict(ldres=97))


def _align_cases():
    """N = 64 + 29 with 96-float pitches, then each route to vec_ok == false alone."""
    for tile, epi in ((6464, 1), (128128, 1), (256128, 1), (256128, 0)):
        for act, res in ((1, 1), (0, 2), (3, 1), (2, 1)):
            for v in ALIGN_VARIANTS:
                kw = dict(ldc=96, ldres=96)
                kw.update(v)
                yield Case("align", "f16x3", tile, epi, E.TILE_BM[tile] + 35, 93, 64, False, act, res, **kw)


BATCH_VARIANTS = (dict(), dict(bias_pb=True), dict(res_shared=True), dict(a2_shared=True), dict(gap=8), dict(gap=5),
                  dict(bias_pb=True, res_shared=True, a2_shared=True, gap=5))


def _batch_cases():
    """Batch 3 through ops.gemm_ex: per-batch / shared bias and residual, a shared addend, a gap between problems, and an sC that is
    not a multiple of 4 on an aligned base (vec_ok differs from one batch index to the next); two folded combinations among them."""
    for tile, epi in ((6464, 1), (256128, 1)):
        for act, res in ((0, 1), (1, 1), (0, 2), (2, 1), (3, 2)):
            for v in BATCH_VARIANTS:
                yield Case("batch", "f16x3", tile, epi, E.TILE_BM[tile] + 35, 93, 64, True, act, res, batch=3, ldc=96, ldres=96, **v)


def _splitk_cases(handmade):
    """splitk_reduce_kernel at all twelve combinations with ldc / ldres wider than N."""
    for act, res in E.COMBOS:
        for splits in (1, 2, 5):
            for M in (1, 25):
                for N in (4, 72):
                    yield Case("reduce" if handmade else "splitk", M=M, N=N, K=32 * splits, a2=not handmade, act=act, res_mode=res,
                               ldc=N + 8, ldres=N + 4, splits=splits, handmade=handmade)


def _ln_cases(handmade):
    """Both LayerNorm reduce kernels on either side of their switch (one workgroup per row up to M = 256, one wave per row beyond);
    splits 1, 4, 5, 9 give the wave kernel's four-at-a-time plane loop 0, 3, 0, 0 leftover planes and 0, 0, 1, 2 full rounds."""
    for M in (256, 257):
        for N in (4, 260, 1024):
            for splits in (1, 4, 5, 9):
                for res, inplace in ((0, False), (1, False), (1, True)):
                    yield Case("reduce" if handmade else "ln", M=M, N=N, K=32 * splits, a2=False, res_mode=res, ldc=N + 8,
                               ldres=N + 4, inplace=inplace, splits=splits, ln=True, handmade=handmade)


def _conv_cases():
    """T = 2, H = 5, W = 7, Cin = 32: 3x3 / stride 1 / pad 1 and 1x1 / stride 2, bias + residual + act 1 / 3, in every mode; the 3x3
    again through the split-K entry with 3 splits -- at N = 36 / 72, the entry takes multiples of 4 only (gemm.hip:571)."""
    for mode in ("f32", "f16x3", "f16"):
        for tile in (6464, 12864, 128128):
            for act in (1, 3):
                for geom in ((2, 5, 7, 32, 3, 1, 1), (2, 5, 7, 32, 1, 2, 0)):
                    for N in (33, 70):
                        yield conv_case(group="conv", mode=mode, tile=tile, N=N, act=act, res_mode=1, conv=geom)
                for N in (36, 72):
                    yield conv_case(group="conv", mode=mode, tile=tile, N=N, act=act, res_mode=1, conv=(2, 5, 7, 32, 3, 1, 1), splits=3)


def _dense_cases():
    """The whole wrapper on dense operands at scale (1, 1), with the addend."""
    for mode in ("f32", "f16x3", "f16"):
        for tile, epi in ((6464, 1), (128128, 1), (256128, 1)):
            N = E.TILE_BN[tile] + 29
            for act, res in ((2, 1), (0, 2), (2, 2), (3, 1)):
                yield Case("dense", mode, tile, epi, E.TILE_BM[tile] + 35, N, 160, True, act, res, ldc=pitch4(N), ldres=pitch4(N),
                           design="dense")


def _act3_cases():
    """act 3 without a residual (rewritten to act 1 by tce_gemm_f32), on both designs."""
    for design in ("exact", "dense"):
        for mode, tile, epi in (("f16x3", 6464, 1), ("f16x3", 256128, 1), ("f16x3", 256128, 0), ("f32", 128128, 1)):
            N = E.TILE_BN[tile] + 29
            yield Case("act3", mode, tile, epi, E.TILE_BM[tile] + 35, N, 64, True, 3, 0, ldc=pitch4(N), design=design)


def _k48_cases():
    """K = 48: not a multiple of the split kernels' 32-wide slice.  Declared in mode f32 -- the arithmetic that must run."""
    for design in ("exact", "dense"):
        for tile in (6464, 12864, 128128):
            N = E.TILE_BN[tile] + 29
            for act, res in ((1, 1), (2, 1), (0, 2)):
                yield Case("k48", "f32", tile, 1, E.TILE_BM[tile] + 35, N, 48, True, act, res, ldc=pitch4(N), ldres=pitch4(N), design=design)


CASES = (list(_instance_cases()) + list(_combo_cases()) + list(_ring_cases()) + list(_align_cases()) + list(_batch_cases())
         + list(_splitk_cases(False)) + list(_ln_cases(False)) + list(_conv_cases()) + list(_splitk_cases(True)) + list(_ln_cases(True))
         + list(_dense_cases()) + list(_act3_cases()) + list(_k48_cases()))


def cases(group, **where):
    return [c for c in CASES if c.group == group and all(getattr(c, k) == v for k, v in where.items())]


# ---------------------------------------------------------------------------------------------------------------------
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
    try:
        ops.check_range()
    except ops.RangeError:
        return True
    return False


@pytest.fixture(autouse=True)
def _range_flag_stays_clean(ops):
    ops.check_range()
    yield
    ops.check_range()   # no case may raise the range flag


_EPI = [1]


def _set_epilogue(lib, form):
    if _EPI[0] != form:
        assert lib.tce_debug_set_epilogue(form) == 0
        _EPI[0] = form


@pytest.fixture(autouse=True)
def _defaults_restored(ops, lib):
    try:
        yield
    finally:
        assert lib.tce_gemm_force_tile(0) == 0
        _set_epilogue(lib, 1)
        assert lib.tce_set_gemm_mode_thread(-1) == 0
        assert lib.tce_set_gemm_mode(1) == 0


@contextmanager
def forced(ops, lib, tile, epi, mode):
    try:
        assert lib.tce_gemm_force_tile(tile) == 0
        _set_epilogue(lib, epi)
        with ops.arith(mode):
            yield
    finally:
        lib.tce_gemm_force_tile(0)
        _set_epilogue(lib, 1)


def _args(c, L, A_, W_, C_, B_, R_, A2_):
    from tce_rvos_amd._lib import GemmArgs
    g = GemmArgs()
    g.A, g.W, g.C, g.bias = A_.data_ptr(), W_.data_ptr(), C_.data_ptr(), B_.data_ptr()
    g.M, g.N, g.K, g.lda, g.ldw, g.ldc = c.M, c.N, c.K, c.K, c.K, L.ldc
    if A2_ is not None:
        g.A2, g.lda2 = A2_.data_ptr(), c.K
    if c.res_mode:
        g.res, g.ldres = R_.data_ptr(), L.ldres
    g.act, g.res_mode, g.batch = c.act, c.res_mode, 1
    return g


def launch(ops, lib, c, o, cb, rb, bb):
    """Issues the case's launch; returns the split-K workspace (or None)."""
    from tce_rvos_amd._lib import check
    L = E.layout(c)
    C_, B_ = cb[L.c_base:], bb[L.b_base:]
    R_ = (cb if c.inplace else rb)[L.r_base:] if c.res_mode else None
    ln = (o.gamma.cuda(), o.beta.cuda()) if c.ln else None
    stream = torch.cuda.current_stream().cuda_stream
    if c.handmade:
        ws = o.planes.cuda().contiguous()
        ops.splitk_reduce(ws, c.splits, c.M, c.N, C_, bias=B_, act=c.act, res=R_, ldres=L.ldres, res_mode=c.res_mode, ln=ln, eps=E.LN_EPS,
                          ldc=L.ldc)
        return None
    ws = torch.full((c.splits * c.M * c.N + E.PAD,), NAN, device="cuda") if c.splits else None
    wsv = ws[:c.splits * c.M * c.N] if c.splits else None
    if c.conv:
        T, H, W, Cin, k, st, p = c.conv
        assert L.ldc == c.N and L.ldres == c.N
        ops.conv2d_cl(o.a.cuda(), o.w.cuda(), T, H, W, Cin, k, k, st, p, bias=B_, act=c.act, out=C_[:c.M * c.N].view(c.M, c.N), res=R_,
                      res_mode=c.res_mode, splitk=c.splits or 1, ws=wsv)
        return ws
    A_, W_ = o.a.cuda().contiguous(), o.w.cuda().contiguous()
    A2_ = o.a2.cuda().contiguous() if c.a2 else None
    if c.splits == 1:   # ops.gemm_ex takes the plain entry at one split: the split-K entries directly
        g = _args(c, L, A_, W_, C_, B_, R_, A2_)
        if c.ln:
            check(lib.tce_gemm_splitk_ln_f32(C.byref(g), 1, ws.data_ptr(), ln[0].data_ptr(), ln[1].data_ptr(), E.LN_EPS, stream),
                  "tce_gemm_splitk_ln_f32")
        else:
            check(lib.tce_gemm_splitk_f32(C.byref(g), 1, ws.data_ptr(), stream), "tce_gemm_splitk_f32")
        return ws
    ops.gemm_ex(A_, W_, C_, c.M, c.N, c.K, c.K, c.K, L.ldc, bias=B_, a2=A2_, lda2=c.K, act=c.act, res=R_, ldres=L.ldres,
                res_mode=c.res_mode, batch=c.batch, sA=c.M * c.K if c.batch > 1 else 0,
                sA2=c.M * c.K if (c.batch > 1 and not c.a2_shared) else 0, sW=0, sBias=L.sBias, sC=L.sC, sRes=L.sRes,
                splitk=max(c.splits, 1), ws=wsv, ln=ln, ln_eps=E.LN_EPS)
    return ws


def run_raw(ops, lib, c, o=None, mode=None):
    """Runs the case; returns its [batch, M, N] outputs after checking that nothing around them was written."""
    o = E.operands(c) if o is None else o
    cbuf, rbuf, bbuf = E.buffers(c, o)
    cb, bb = cbuf.cuda(), bbuf.cuda()
    rb = rbuf.cuda() if rbuf is not None else None
    with forced(ops, lib, c.tile, c.epi, mode or c.mode):
        ws = launch(ops, lib, c, o, cb, rb, bb)
        torch.cuda.synchronize()
    flat = cb.cpu()
    idx = E.out_index(c)
    around = torch.ones(flat.numel(), dtype=torch.bool)
    around[idx.flatten()] = False
    assert bool(flat[around].isnan().all()), f"{c.label}: {int((~flat[around].isnan()).sum())} elements around the outputs were written"
    if ws is not None:
        assert bool(ws[-E.PAD:].isnan().all()), f"{c.label}: the launch wrote past its partial planes"
    if rb is not None:
        assert torch.equal(rb.cpu().nan_to_num(7.0), rbuf.nan_to_num(7.0)), f"{c.label}: the residual buffer was written"
    return flat[idx]


def run_case(ops, lib, c):
    o = E.operands(c)
    out = run_raw(ops, lib, c, o)
    ref, B = E.reference(c, o)
    print(f"{c.label}: ", end="")
    kind, r = E.compare(c, out, ref, B)
    print("exact" if kind == "exact" else f"err/B {r:.3f}")
    RESULTS.append((c, kind, r))
    return out


def run_all(ops, lib, which):
    assert which, "no case selected"
    failures = []
    for c in which:
        try:
            run_case(ops, lib, c)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, f"{len(failures)} of {len(which)} cases:\n" + "\n".join(failures[:10])


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tile,epi", SPLIT_INSTANCES + F32_INSTANCES)
@pytest.mark.parametrize("a2", [False, True])
def test_kernel_instance(ops, lib, mode, tile, epi, a2):
    run_all(ops, lib, cases("instance", mode=mode, tile=tile, epi=epi, a2=a2))


@pytest.mark.parametrize("mode,tile,epi", [("f16x3", 6464, 1), ("f32", 6464, 1), ("f16x3", 256128, 1), ("f16x3", 256128, 0),
                                           ("f16", 256128, 1)])
def test_all_twelve_combinations(ops, lib, mode, tile, epi):
    run_all(ops, lib, cases("combo", mode=mode, tile=tile, epi=epi))


@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_one_slice_ring_at_512_workgroups(ops, lib, mode):
    run_all(ops, lib, cases("ring", mode=mode))


@pytest.mark.parametrize("tile,epi", [(6464, 1), (128128, 1), (256128, 1), (256128, 0)])
def test_unaligned_routes_are_bit_identical(ops, lib, tile, epi):
    """Aligned, then C / bias / residual base + 4 bytes, ldc odd, ldres odd, each alone: all six results hold the same bits (the
    GELU combination too: the same operations on the same values) and meet the expectation."""
    for act, res in ((1, 1), (0, 2), (3, 1), (2, 1)):
        group = cases("align", tile=tile, epi=epi, act=act, res_mode=res)
        assert len(group) == len(ALIGN_VARIANTS)
        outs = [run_case(ops, lib, c) for c in group]
        for c, out in zip(group[1:], outs[1:]):
            assert torch.equal(out, outs[0]), f"{c.label}: differs from the aligned launch"


@pytest.mark.parametrize("tile,epi", [(6464, 1), (256128, 1)])
def test_batch_strides(ops, lib, tile, epi):
    run_all(ops, lib, cases("batch", tile=tile, epi=epi))


@pytest.mark.parametrize("tile", [6464, 256128])
def test_folded_combinations_are_rejected_in_place(ops, lib, tile):
    """The four combinations that need epi_fix_kernel read the residual after the GEMM stored over it: TceError in place.  (The
    fifth combination without a fused body, act 3 / res 0, has no residual to alias: it is rewritten to act 1, next test.)"""
    from tce_rvos_amd._lib import TceError
    base = Case("combo", "f16x3", tile, 1, 70, 72, 32, False, inplace=True)
    for act, res in E.FOLDED:
        c = E.replace(base, act=act, res_mode=res)
        with pytest.raises(TceError):
            run_raw(ops, lib, c)


@pytest.mark.parametrize("design", ["exact", "dense"])
def test_act3_without_residual_is_act1(ops, lib, design):
    """act = 3, res_mode = 0 is rewritten to act = 1 (gemm.hip:340): the same bits."""
    for c3 in cases("act3", design=design):
        out3, out1 = run_case(ops, lib, c3), run_raw(ops, lib, E.replace(c3, act=1))
        assert torch.equal(out3, out1), c3.label
        assert float(out3.min()) == 0.0 and float(out3.max()) > 0.0


@pytest.mark.parametrize("tile", [6464, 12864, 128128])
@pytest.mark.parametrize("design", ["exact", "dense"])
def test_k48_falls_back_to_the_fp32_kernel(ops, lib, tile, design):
    """K % 32 != 0 in mode f16x3 runs the exact-fp32 kernel (gemm.hip:351): the same bits as mode f32, inside mode f32's bound."""
    for c in cases("k48", tile=tile, design=design):
        out32, out = run_case(ops, lib, c), run_raw(ops, lib, c, mode="f16x3")
        assert torch.equal(out, out32), f"{c.label}: mode f16x3 at K = 48 differs from mode f32"


def test_splitk_reduce_all_combinations(ops, lib):
    run_all(ops, lib, cases("splitk"))


@pytest.mark.parametrize("M", [256, 257])
def test_layernorm_reduce(ops, lib, M):
    run_all(ops, lib, cases("ln", M=M))


def test_standalone_reduce_on_handmade_planes(ops, lib):
    run_all(ops, lib, cases("reduce"))


@pytest.mark.parametrize("mode", ["f32", "f16x3", "f16"])
def test_implicit_gemm_convolution(ops, lib, mode):
    run_all(ops, lib, cases("conv", mode=mode))


def test_splitk_entry_takes_multiples_of_four_only(ops, lib):
    from tce_rvos_amd._lib import TceError
    with pytest.raises(TceError):
        run_raw(ops, lib, conv_case(group="conv", tile=6464, N=33, act=1, res_mode=1, conv=(2, 5, 7, 32, 3, 1, 1), splits=3))


@pytest.mark.parametrize("mode", ["f32", "f16x3", "f16"])
def test_dense_wrapper(ops, lib, mode):
    run_all(ops, lib, cases("dense", mode=mode))


def test_range_flag_sees_only_rows_that_are_stored(ops, lib):
    """include/tce_rvos.h: the flag reports what is STORED.  Rows >= M of the 256128 tile's last 32-row fragment evaluate
    (0 + bias) * (the last valid row's residual) = 90000 here; every stored value is O(1)."""
    c, o = E.range_probe()
    ref, _ = E.reference(c, o)
    assert float(ref.abs().max()) < 3000.0 and 300.0 * 300.0 >= E.RANGE_LIMIT
    for mode in ("f16x3", "f16"):
        out = run_raw(ops, lib, c, o, mode=mode)
        flag = raised(ops)
        assert torch.equal(out, ref)
        assert not flag, f"mode {mode}: the range flag was raised by values of rows >= M that are never stored"


# ---------------------------------------------------------------------------------------------------------------------
def test_zz_defaults_are_back(ops, lib):
    """Forced tile, epilogue form and arithmetic mode are at their defaults: the launcher's own choices again."""
    assert ops.get_gemm_mode() == "f16x3"
    assert lib.tce_gemm_select_tile_ex(130, 70, 96, 1, 0) == 6464
    assert lib.tce_gemm_select_tile_ex(49100, 256, 32, 1, 0) == 256128
    assert lib.tce_gemm_select_tile_ex(2 * 45 * 81, 250, 576, 1, 1) == 6464
    assert _EPI[0] == 1


def test_zz_write_profile():
    """One line per case (run the whole module: every test above appends its cases)."""
    ran = {c for c, _, _ in RESULTS}
    missing = [c.label for c in CASES if c not in ran]
    assert not missing, f"{len(missing)} cases did not run, e.g. {missing[:3]}"
    worst = {}
    for c, kind, r in RESULTS:
        if kind == "bound":
            worst[c.instance] = max(worst.get(c.instance, 0.0), r)
    with open(PROFILE, "w") as f:
        f.write("# tests/test_gemm_epilogue_gpu.py on an MI355X: per case, 'exact' (the stored bits equal the fp32 chain of gemm_epilogue.h on the\n"
                "# exact-product design) or the worst |out - fp64 ref| / B over the outputs (GELU, LayerNorm and the dense design).\n"
                "# instance and tile | shape | combination | alignment variant | result\n")
        seen = set()
        for c, kind, r in RESULTS:
            if c in seen:
                continue
            seen.add(c)
            f.write(f"{c.label} | {'exact' if kind == 'exact' else f'{r:.3f}'}\n")
        f.write("# worst err/B per instance\n")
        for inst in sorted(worst):
            f.write(f"# {inst} | {worst[inst]:.3f}\n")
