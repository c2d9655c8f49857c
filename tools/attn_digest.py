"""The outputs of the attention kernels (csrc/attn.hip, swinattn.hip) and of the thin GEMM (thin.hip) as text, for diffing two
trees: per case one line, the SHA-256 of the output bytes and the case name.  Inputs are seeded, every launch goes through ops,
and nothing but outputs is looked at.  Two trees whose kernels compute the same bits print the same lines.
    python tools/attn_digest.py [--root TREE] [--only SUBSTRING] > digest.txt
--root: the tree whose package is run (default: this one), so one file serves both sides of a comparison.
Cases are the smallest that reach each code path: every launch form of mha_core (tests/_attn.py CASES, with and without a key
mask; the form is asserted as the tests assert it), 2-D and 3-D windows under every arithmetic and every kernel switch, the
fused Swin attention block, and one thin_partials + splitk_reduce."""
import argparse
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(HERE))
ap.add_argument("--only", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))  # the inputs come from this tree's tests/_attn.py for both sides
sys.path.insert(0, os.path.abspath(a.root))
import torch  # noqa: E402
import _attn as AT  # noqa: E402
from tce_rvos_amd import ops  # noqa: E402
from tce_rvos_amd._lib import lib  # noqa: E402

MODES = ("f32", "f16x3", "f16")


def emit(name, *outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    print(f"{h.hexdigest()}  {name}", flush=True)


def wanted(name):
    return a.only in name


def randn(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def alloc(n):
    return torch.empty(n, dtype=torch.float32, device="cuda")


def mha():
    for name, batch, nh, Lq, Lk, ws, modes in AT.CASES:
        E = nh * 32
        q, k, v = (t.cuda() for t in AT.operands("N", batch, nh, Lq, Lk, seed=1))
        for mask_name, build in (("no mask", AT.mask_m0), ("M2", AT.mask_m2)):
            mask = build(batch, Lk)
            for mode in modes:
                title = f"mha_core {name} [{mode}] {mask_name}"
                if not wanted(title):
                    continue
                ops.set_gemm_mode(mode)
                form = AT.mha_form(batch, nh, Lq, Lk, mode, ws)
                assert form == name[:2], f"{title}: selects {form}"
                out = torch.zeros(batch, Lq, E, device="cuda")
                ops.mha_core(q, k, v, batch, nh, Lq, Lk, E, E, E, Lq * E, Lk * E, Lk * E, out, E, Lq * E,
                             kmask=None if mask is None else mask.cuda(), alloc=alloc if ws else None)
                emit(f"{title} ({form})", out)


def windows2d():
    for T, H, W, nH, shift in ((2, 18, 25, 3, 0), (2, 18, 25, 3, 3), (1, 7, 7, 1, 3), (3, 5, 7, 2, 3)):
        C = nH * 32
        qkv, b, tab = randn(2, T * H * W, 3 * C), randn(3, 3 * C), randn(4, 13 * 13, nH)
        for mode in MODES:
            for switch in (0, 1, 2):
                title = f"window_attn T{T} {H}x{W} nH{nH} shift{shift} [{mode}] switch {switch}"
                if not wanted(title):
                    continue
                ops.set_gemm_mode(mode)
                lib().tce_debug_window_attn_set_mfma(switch)
                emit(title, ops.window_attn(qkv, b, tab, T, H, W, C, nH, shift, out=torch.zeros(T * H * W, C, device="cuda")))


def windows3d():
    for T, H, W, nH, shifted in ((3, 18, 25, 3, False), (3, 18, 25, 3, True), (9, 3, 4, 2, True), (17, 8, 6, 1, True)):
        C = nH * 32
        qkv, b, tab = randn(5, T * H * W, 3 * C), randn(6, 3 * C), randn(7, 15 * 13 * 13, nH)
        for mode in MODES:
            for switch in (0, 1):
                title = f"window_attn3d T{T} {H}x{W} nH{nH} shifted={shifted} [{mode}] switch {switch}"
                if not wanted(title):
                    continue
                ops.set_gemm_mode(mode)
                lib().tce_debug_window_attn_set_mfma(switch)
                emit(title, ops.window_attn3d(qkv, b, tab, T, H, W, C, nH, shifted, out=torch.zeros(T * H * W, C, device="cuda")))


def swin_fused():
    for T, H, W, C, shift in ((2, 18, 25, 96, 3), (1, 9, 13, 192, 3), (1, 7, 7, 128, 0)):
        nH = C // 32
        x, wqkv, wp = randn(8, T * H * W, C), randn(9, 3 * C, C, scale=C ** -0.5), randn(10, C, C, scale=C ** -0.5)
        bqkv, bp, tab = randn(11, 3 * C, scale=0.1), randn(12, C, scale=0.1), randn(13, 13 * 13, nH)
        g1, b1 = 1.0 + randn(14, C, scale=0.1), randn(15, C, scale=0.1)
        for mode in ("f16x3", "f16"):
            title = f"swin_attn_fused T{T} {H}x{W} C{C} shift{shift} [{mode}]"
            if not wanted(title):
                continue
            ops.set_gemm_mode(mode)
            pk = ops.swin_attn_pack(wqkv, wp)  # the stream carries the mode's rounding
            emit(title, ops.swin_attn_fused(x, pk, bqkv, bp, tab, g1, b1, T, H, W, C, shift, out=torch.zeros(T * H * W, C, device="cuda")))


def thin():
    M, N, K = 32, 768, 3072
    title = f"thin_partials + splitk_reduce {M}x{N}x{K} [f16x3]"
    if not wanted(title):
        return
    ops.set_gemm_mode("f16x3")
    x, w = randn(16, M, K), randn(17, N, K, scale=K ** -0.5)
    splits = ops.thin_splits(M, N, K)
    assert splits == K // 256, f"{title}: not a thin shape ({splits} planes)"
    ws = ops.thin_partials(x, w, torch.zeros(splits, M, N, device="cuda"), M, N, K)
    emit(title, ws, ops.splitk_reduce(ws, splits, M, N, torch.zeros(M, N, device="cuda")))


try:
    mha()
    windows2d()
    windows3d()
    swin_fused()
    thin()
finally:
    lib().tce_debug_window_attn_set_mfma(1)
    ops.set_gemm_mode("f16x3")
