"""CPU: the operands and bounds of test_arith_bound_gpu.py discriminate, shown on an emulation of the split-fp16 arithmetic with no
kernel involved.  For every (K, weight scale, activation scale) of the GPU module the correct emulated arithmetic (truncating and
round-to-nearest halves) is inside the bound B on every element, and every defect the GPU module claims to catch is at least
4 x outside it on some element.  The 4 x is a condition on the CHOICE OF INPUTS, checked here; the bound itself has no margin."""
import math

import pytest
import torch

import _arith as A

N_COLS = 64
MARGIN = 4.0


def _ratio(out, ref, B):
    err = (out.double() - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / B).max().item()   # an exact result is inside any bound, B = 0 included


@pytest.mark.parametrize("K", A.DENSE_K)
def test_dense_correct_arithmetic_is_inside_the_bound(K):
    M = 128 if K <= 3072 else 32
    for ws, as_ in A.DENSE_SCALES:
        a, w = A.dense_operands(M, N_COLS, K, ws, as_, seed=K)
        ref = a.double() @ w.double().T
        B = A.bound_split(a, w, A.c_dense(K))
        for rtz in (True, False):
            r = _ratio(A.emulate_split(a, w, rtz), ref, B)
            assert r <= 1.0, (K, ws, as_, rtz, r)
        # mode "f16" and the exact-fp32 bound hold their own arithmetic too
        assert _ratio(A.emulate_split(a, w, mutant="single_pass"), ref, A.bound_f16(a, w, A.c_dense(K))) <= 1.0
        assert _ratio(a @ w.T, ref, A.bound_f32(a, w)) <= 1.0
    a, w = A.decades_operands(M, N_COLS, K, seed=K)
    ref = a.double() @ w.double().T
    for rtz in (True, False):
        assert _ratio(A.emulate_split(a, w, rtz), ref, A.bound_split(a, w, A.c_dense(K))) <= 1.0


@pytest.mark.parametrize("K", [k for k in A.DENSE_K if 32 <= k <= 2048])
def test_dense_sweep_sees_global_defects_at_ordinary_magnitude(K):
    """A cross term dropped everywhere: >= 4 x outside the dense bound at unit scale and at (2^4, 2^4), for 32 <= K <= 2048.  Subnormal
    lo values flushed to zero: claimed at unit scale from K = 128 up, where most weights (~ 1 / sqrt(K)) lie below 2^-3 and so have a
    subnormal lo; at (2^4, 2^4) hardly any operand has one and nothing is claimed.  A single pass in place of three: claimed for
    K <= 768; it rounds to nearest, so its random-sign error is half the truncating forms' and at K = 2048 the emulation leaves it
    just under 4 x (the probe sees it at >= 20 x at every K).
    NOT asserted, because the contract's absolute floor 2^-24 is then most of B and hides a dropped term: weights x 2^-4 at large K
    (1.1 x B at K = 2048), weights x 2^-8 at any K (0.6 x B at K = 256), activations x 2^-8 at K = 2048 (2.2 x B); there the probe
    carries the check.  K = 16: too few terms for a random-sign sum to stand clear of the worst-case B, so the claim starts at 32."""
    M = 128
    for ws, as_ in ((1.0, 1.0), (16.0, 16.0)):
        a, w = A.dense_operands(M, N_COLS, K, ws, as_, seed=K + 1)
        ref = a.double() @ w.double().T
        B = A.bound_split(a, w, A.c_dense(K))
        claimed = ["drop_alo_whi", "drop_ahi_wlo"]
        if ws == 1.0 and K >= 128:
            claimed.append("flush_subnormal_lo")
        if K <= 768:
            claimed.append("single_pass")
        for m in claimed:
            r = _ratio(A.emulate_split(a, w, True, m), ref, B)
            assert r >= MARGIN, (K, ws, as_, m, r)


@pytest.mark.parametrize("K,period", [(K, p) for K in A.PROBE_K for p in (128, 256) if K <= 768 or p == 256])
def test_probe_correct_inside_and_local_defects_outside(K, period):
    M = A.probe_rows(K, period)
    for ws, as_ in A.PROBE_SCALES:
        a = A.kblock_probe(M, K, as_, period, seed=K)
        _, w = A.dense_operands(1, N_COLS, K, ws, 1.0, seed=K + 7)
        ref = a.double() @ w.double().T
        B = A.bound_split(a, w, A.c_probe(a))
        for rtz in (True, False):
            r = _ratio(A.emulate_split(a, w, rtz), ref, B)
            assert r <= 1.0, (K, ws, as_, rtz, r)
        for m in A.LOCAL_MUTANTS + A.GLOBAL_MUTANTS:
            if m == "wlo_misplaced_frag" and ws / math.sqrt(K) < 2.0 ** -9:
                # weights ~ 2^-9.5 and below: lo < 2^-11 |w| sits within 4 bits of the 2^-24 quantum, so ONE misplaced fragment of ONE
                # weight row (seen by the ~30 rows of its block in one column) need not stand 4 x clear of the floor; not claimed
                continue
            r = _ratio(A.emulate_split(a, w, True, m), ref, B)
            assert r >= MARGIN, (K, ws, as_, m, r)
        # the mode switch is real: single-pass arithmetic is inside ITS bound and outside the split bound
        one = A.emulate_split(a, w, mutant="single_pass")
        assert _ratio(one, ref, A.bound_f16(a, w, A.c_probe(a))) <= 1.0


@pytest.mark.parametrize("T,H,W,Cin,k,s,p", [(1, 9, 7, 64, 3, 1, 1), (3, 12, 20, 64, 3, 2, 1), (2, 14, 10, 256, 1, 2, 0), (3, 17, 5, 256, 3, 1, 1),
                                             (5, 12, 20, 768, 3, 2, 1)])
def test_conv_probe_design_discriminates(T, H, W, Cin, k, s, p):
    """The convolution probes of the GPU module (one channel block per frame, non-zero pixels on a lattice of pitch 3): every
    output row has at most 8 non-zeros, all of one tap; every tap and every channel block occurs; the correct arithmetic is inside
    B and the local and global defects are >= 4 x outside (same exception as the linear probe for one misplaced fragment of tiny
    weights).  The dense and four-decade convolution cases are dense products of K = k*k*Cin, covered by DENSE_K above."""
    for kind, ws, as_, Tn, x, w in A.conv_cases(T, H, W, Cin, N_COLS, k, seed=3):
        if kind != "probe":
            continue
        a = A.im2col(x, Tn, H, W, Cin, k, s, p)
        nz = a != 0
        assert int(nz.sum(1).max()) <= 8
        first = nz.float().argmax(1)[nz.any(1)]
        assert set((first // Cin).tolist()) == set(range(k * k)) and set((first % Cin // 8).tolist()) == set(range(Cin // 8))
        ref = a.double() @ w.double().T
        B = A.bound_split(a, w, A.c_probe(a))
        for rtz in (True, False):
            assert _ratio(A.emulate_split(a, w, rtz), ref, B) <= 1.0
        for m in A.LOCAL_MUTANTS + A.GLOBAL_MUTANTS:
            if m == "wlo_misplaced_frag" and ws / math.sqrt(k * k * Cin) < 2.0 ** -9:
                continue
            r = _ratio(A.emulate_split(a, w, True, m), ref, B)
            assert r >= MARGIN, (ws, as_, m, r)


def test_probe_covers_every_block_and_row_in_tile():
    for K, period in ((96, 128), (256, 256), (384, 128)):
        M = A.probe_rows(K, period)
        blk = A.probe_blocks(M, K, period)
        pairs = set(zip((torch.arange(M) % period).tolist(), blk.tolist()))
        assert len(pairs) == period * (K // 8)
    for K, period in ((2304, 128), (3072, 256)):   # capped row count: every block still occurs
        assert set(A.probe_blocks(A.probe_rows(K, period), K, period).tolist()) == set(range(K // 8))
    # shifted launches (families with few rows by nature): K / 8 launches of R rows put every block in every row
    R, K = 32, 768
    seen = set()
    for s in range(K // 8):
        seen |= set(zip(range(R), A.probe_blocks(R, K, 256, shift=s).tolist()))
    assert len(seen) == R * (K // 8)


def test_chosen_tails_keep_the_first_order_bound_meaningful():
    """No LayerNorm row of the GPU module's dense inputs has sigma < 1e-3, and no GELU argument lies beyond +-6: randn rows of >= 48
    channels at every activation scale of the sweep, after a unit-variance product."""
    for C in (48, 96, 256):
        for _, as_ in A.DENSE_SCALES:
            a, w = A.dense_operands(512, C, C, 1.0, as_, seed=C)
            z = a.double() @ w.double().T
            if as_ >= 1.0 / 16:
                assert A.layernorm_sigma(z).min().item() > 1e-3
            assert z.abs().max().item() < 6.0 * max(1.0, as_ * 16)
    x = torch.linspace(-6, 6, 20001, dtype=torch.float64)
    dg = 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi)
    assert dg.abs().max().item() <= A.GELU_LIPSCHITZ


def test_layernorm_bound_is_first_order_correct():
    g = torch.Generator().manual_seed(1)
    z = torch.randn(64, 256, generator=g, dtype=torch.float64) * 3 + 0.5
    gam = torch.rand(256, generator=g, dtype=torch.float64) + 0.5
    dz = torch.rand(64, 256, generator=g, dtype=torch.float64) * 1e-6
    sgn = torch.sign(torch.randn(64, 256, generator=g, dtype=torch.float64))
    ln = lambda t: torch.nn.functional.layer_norm(t, (256,), gam, None, 1e-5)
    d = (ln(z + sgn * dz) - ln(z)).abs()
    assert (d <= 1.01 * A.layernorm_bound(z, dz, gam, 1e-5)).all()


@pytest.mark.parametrize("C,Hd", [(96, 384), (128, 512), (192, 768), (256, 2048), (256, 64)])
@pytest.mark.parametrize("which", ["first", "second"])
def test_ffn_probe_design_discriminates(C, Hd, which):
    """The fused-FFN probes of the GPU module (two chained products, ReLU as the identity): the correct emulated chain is inside the
    composed bound, one lost k index of the probed product's lo is >= 4 x outside, and so is a single pass."""
    M = A.probe_rows(C, 256)
    for j, (ws, as_) in enumerate(A.PROBE_SCALES):
        x, w1, b1, w2, b2, c1, c2 = A.ffn_probe_operands(which, C, Hd, M, 256, ws, as_, seed=C + Hd + j)
        ref, B, S, h = A.ffn_ref_and_bound(x, w1, b1, w2, b2, "relu", None, None, c1, c2)
        assert bool((h >= 0).all())

        def chain(m1, m2):
            hid = torch.relu(A.emulate_split(x, w1, True, m1))
            return x + A.emulate_split(hid, w2, True, m2)
        assert _ratio(chain(None, None), ref, B) <= 1.0
        local = ("lo_zero_one_k", None) if which == "first" else (None, "lo_zero_one_k")
        # activations x 2^-8: x's lo keeps 5 bits above the 2^-24 quantum and the composed bound carries the factor 2 of the
        # second-order remainder, so one lost lo stands 4 - 9 x clear, not always 4: the claim there is 2 x
        need = MARGIN if as_ == 1.0 else 2.0
        assert _ratio(chain(*local), ref, B) >= need, (ws, as_, _ratio(chain(*local), ref, B))
        assert _ratio(chain("single_pass", "single_pass"), ref, B) >= MARGIN
