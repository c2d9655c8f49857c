"""Capped (persistent) launches of the fused FFN / folded cross-attention (csrc/ffn.hip PERSIST, tce_ffn_set_wg_cap, ops.ffn_wg_cap,
TCE_LAT1_CUS / TCE_LAT1_AT): a capped launch runs the same blocks on fewer workgroups, so every check here is BIT identity against
the uncapped launch -- no tolerance.  Rows: 5 * 128 + 37 = six 128-row blocks, the last ragged."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

M, CN = 5 * 128 + 37, 256
CAPS = (1, 2, 4, 6, 64)  # 6 and 64 >= the six blocks: the plain launch
CANARY = 0x7FC0DEAD      # a NaN with a payload: rows the launch must not write keep exactly these bits


# --------------------------------------------------------------------------------------------------------------- CPU
def _plan(cap, batch, blocks):
    """The launcher's rule restated: no cap, or a launch that stays inside it -> one workgroup per block; else max(1, cap / batch)
    persistent workgroups per batch entry -- unless that is every block anyway."""
    if cap <= 0 or blocks * batch <= cap:
        return blocks, 0
    gx = max(1, cap // batch)
    return (blocks, 0) if gx >= blocks else (gx, 1)


def test_cap_entries_launch_nothing():
    from tce_rvos_amd import _lib, hazard
    for name in ("tce_ffn_set_wg_cap", "tce_ffn_capped_grid"):
        assert name in _lib.SIGNATURES and name in hazard.NOT_LAUNCHES and name not in hazard.MODELS


def test_capped_grid_arithmetic_matches_restatement():
    from tce_rvos_amd import _lib
    l = _lib.lib()
    seen = set()
    for cap in (0, 1, 2, 3, 4, 6, 7, 32, 48, 64, 96, 128, 562, 563, 564, 4000):
        for batch in (1, 2, 3, 5, 8, 40):
            for blocks in (1, 2, 5, 6, 7, 63, 189, 563, 1000):
                p = ctypes.c_int32(-1)
                gx = l.tce_ffn_capped_grid(cap, batch, blocks, ctypes.byref(p))
                assert (gx, p.value) == _plan(cap, batch, blocks), (cap, batch, blocks)
                assert 1 <= gx <= blocks and (p.value == 0) == (gx == blocks)  # never more workgroups than blocks
                seen.add(p.value)
    assert seen == {0, 1}
    assert l.tce_ffn_capped_grid(64, 1, 563, None) == 64  # the stride-4 launches of config 2
    assert l.tce_ffn_set_wg_cap(-1) != 0 and l.tce_ffn_set_wg_cap(0) == 0


# --------------------------------------------------------------------------------------------------------------- kernels
@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tce_rvos_amd import ops as _ops
    _ops.range_flag()["flag"].zero_()  # registered with the library before the first launch
    return _ops


def _randn(g, *shape, s=1.0):
    return (torch.randn(*shape, generator=g) * s).cuda().contiguous()


def _flag(ops):
    torch.cuda.synchronize()
    f = ops.range_flag()["flag"]
    v = int(f.item())
    f.zero_()
    return v


def _padded(rows_t, extra=128):
    """[M + extra, 256] buffer, the rows past M filled with the canary bits; returns (buffer, its first M rows)."""
    buf = torch.full((M + extra, CN), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)
    if rows_t is not None:
        buf[:M] = rows_t
    return buf, buf[:M]


def _canary_ok(buf):
    return bool((buf[M:].view(torch.int32) == CANARY).all())


@pytest.fixture(scope="module")
def ffn_data(ops):
    g = torch.Generator().manual_seed(1234)
    d = {"x": _randn(g, M, CN), "gi": _randn(g, CN, s=0.2) + 1, "bi": _randn(g, CN, s=0.2), "go": _randn(g, CN, s=0.2) + 1,
         "bo": _randn(g, CN, s=0.2), "b2": _randn(g, CN, s=0.2)}
    for hd in (64, 2048):
        d[hd] = (_randn(g, hd, CN, s=1 / 16), _randn(g, hd, s=0.2), _randn(g, CN, hd, s=hd ** -0.5))
    return d


@gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16"])
@pytest.mark.parametrize("hd", [64, 2048])
def test_plain_ffn_capped_is_bit_identical(ops, ffn_data, hd, mode):
    """Out of place without LayerNorms, and in place (out = x, the residual) with LayerNorm in and out.  (The plain entry has no
    separate `res` / `a2`: those operands are covered through the cross-attention entry below, the same kernel.)"""
    d = ffn_data
    with ops.arith(mode):
        pk = ops.ffn_pack(*d[hd])

        def run(cap, inplace):
            with ops.ffn_wg_cap(cap):
                if inplace:
                    buf, x = _padded(d["x"])
                    ops.ffn_fused(x, pk, d["b2"], hd, ops.ACT_RELU, ln_in=(d["gi"], d["bi"]), ln_out=(d["go"], d["bo"]), M=M)
                    return buf, x
                buf, out = _padded(None)
                ops.ffn_fused(d["x"], pk, d["b2"], hd, ops.ACT_RELU, out=out, M=M)
                return buf, out
        for inplace in (False, True):
            _, ref = run(0, inplace)
            flag0 = _flag(ops)
            assert flag0 == 0 and bool(torch.isfinite(ref).all())
            for cap in CAPS:
                buf, out = run(cap, inplace)
                assert _flag(ops) == flag0
                assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), (cap, inplace)
                assert _canary_ok(buf), (cap, inplace)


@pytest.fixture(scope="module")
def xattn_data(ops):
    g = torch.Generator().manual_seed(4321)
    d = {"x": _randn(g, 2 * M, CN), "res": _randn(g, 2 * M, CN), "pos": _randn(g, 97, CN, s=0.5), "bo": _randn(g, CN, s=0.2),
         "g": _randn(g, CN, s=0.2) + 1, "b": _randn(g, CN, s=0.2)}
    wq, bq, wo = _randn(g, CN, CN, s=0.06), _randn(g, CN, s=0.2), _randn(g, CN, CN, s=0.06)
    d["wqT"], d["wo"] = ops.xattn_static(wq, bq), wo
    for group, L in ((32, 11), (8, 8)):
        d[group] = (_randn(g, 2 * L, CN), _randn(g, 2 * L, CN), L)
    return d


@gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16"])
@pytest.mark.parametrize("group", [32, 8])  # ACT 3 (32 key slots per head) and ACT 4 (8)
def test_xattn_fold_capped_is_bit_identical(ops, xattn_data, group, mode):
    """a2 with a2_rows (a 97-row position map, row index modulo 97), a separate multiplicative `res`, LayerNorm out in place, and
    two batch entries with a weight stream each: the cap divides over grid.y (cap 4 -> two workgroups per entry, cap 1 -> one)."""
    d = xattn_data
    k, v, L = d[group]
    alloc = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="cuda")  # noqa: E731
    with ops.arith(mode):
        pk = ops.xattn_pack(k, v, d["wqT"], d["wo"], L, alloc, group=group, batch=2)
        variants = {
            "a2_rows+ln, in place": lambda x, out: ops.xattn_fused(x, pk[0], d["bo"], M, x, a2=d["pos"], a2_rows=97, ln_out=(d["g"], d["b"]),
                                                                   group=group),
            "separate res, multiply": lambda x, out: ops.xattn_fused(x, pk[0], d["bo"], M, out, res=d["res"], res_mode=ops.RES_MUL,
                                                                     group=group),
            "separate res, add, a2": lambda x, out: ops.xattn_fused(x, pk[0], d["bo"], M, out, a2=d["pos"], a2_rows=97, res=d["res"],
                                                                    ln_out=(d["g"], d["b"]), group=group),
        }
        for name, fn in variants.items():
            outs = {}
            for cap in (0,) + CAPS:
                xb, x = _padded(d["x"][:M])
                ob, out = _padded(None)
                with ops.ffn_wg_cap(cap):
                    fn(x, out)
                res = x if "in place" in name else out
                outs[cap] = (res.clone(), _flag(ops))
                assert _canary_ok(xb) and _canary_ok(ob), (name, cap)
            assert outs[0][1] == 0 and bool(torch.isfinite(outs[0][0]).all())
            for cap in CAPS:
                assert outs[cap][1] == outs[0][1] and torch.equal(outs[cap][0].view(torch.int32), outs[0][0].view(torch.int32)), (name, cap)
        # batch 2, per-batch weight streams, entries M rows apart in one [2M, 256] tensor, in place
        outs = {}
        for cap in (0, 1, 2, 3, 4, 5, 11, 12, 64):
            x = d["x"].clone()
            with ops.ffn_wg_cap(cap):
                ops.xattn_fused(x, pk, d["bo"], M, x, a2=d["pos"], a2_rows=97, ln_out=(d["g"], d["b"]), batch=2, sX=M * CN, sOut=M * CN,
                                group=group, per_batch_weights=True)
            outs[cap] = x
            assert _flag(ops) == 0
        assert not torch.equal(outs[0][:M], outs[0][M:])
        for cap, x in outs.items():
            assert torch.equal(x.view(torch.int32), outs[0].view(torch.int32)), ("batch 2", cap)


@gpu
@pytest.mark.parametrize("kind", ["ffn", "xattn"])
def test_capped_blocks_start_cold(ops, ffn_data, xattn_data, kind):
    """What a block leaves behind must not reach the next one on the same workgroup.  By data, not timing: blocks 0, 2 and 4 are
    rows of NaN / Inf / 6e4-sized values -- at the end of such a block the accumulators, the hidden-chunk fragments, the staging tile
    and the range maximum all hold them -- and blocks 1, 3, 5 are ordinary rows.  With cap 1 one workgroup walks all six in turn,
    with cap 2 one takes the poisoned and one the clean blocks, with cap 4 two workgroups run two blocks each.  Run twice over a
    NaN-filled `out`: the clean blocks' rows must be the uncapped launch's bits (finite), the poisoned rows the uncapped launch's
    bits too, nothing past row M written, and the range flag what the uncapped launch raises (set here; clear on clean data)."""
    g = torch.Generator().manual_seed(77)
    x0 = (ffn_data["x"] if kind == "ffn" else xattn_data["x"][:M]).clone()
    for blk in (0, 2, 4):
        rows = x0[blk * 128:(blk + 1) * 128]
        rows[0::3] = float("nan")
        rows[1::3] = float("inf")
        rows[2::3] = torch.randn(rows[2::3].shape, generator=g).cuda() * 6e4
    clean = torch.zeros(M, dtype=torch.bool, device="cuda")
    for blk in (1, 3, 5):
        clean[blk * 128:(blk + 1) * 128] = True
    if kind == "ffn":
        pk = ops.ffn_pack(*ffn_data[2048])
        launch = lambda x, out: ops.ffn_fused(x, pk, ffn_data["b2"], 2048, ops.ACT_RELU, ln_out=(ffn_data["go"], ffn_data["bo"]), out=out, M=M)  # noqa: E731
    else:
        d = xattn_data
        k, v, L = d[32]
        alloc = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="cuda")  # noqa: E731
        pk = ops.xattn_pack(k[:L], v[:L], d["wqT"], d["wo"], L, alloc)
        launch = lambda x, out: ops.xattn_fused(x, pk, d["bo"], M, out, a2=d["pos"], a2_rows=97, ln_out=(d["g"], d["b"]))  # noqa: E731
    xb, x = _padded(x0)  # garbage (canary NaNs) behind row M of the input as well
    res = {}
    for cap in (0, 1, 2, 4):
        ob, out = _padded(None)
        out.fill_(float("nan"))
        with ops.ffn_wg_cap(cap):
            launch(x, out)
            first = out.clone()
            f1 = _flag(ops)
            launch(x, out)
        res[cap] = (out.clone(), f1, _flag(ops))
        assert torch.equal(first.view(torch.int32), out.view(torch.int32)), cap  # the second run over the first one's results
        assert _canary_ok(ob) and _canary_ok(xb), cap
    ref = res[0][0]
    assert bool(torch.isfinite(ref[clean]).all()) and not bool(torch.isfinite(ref[~clean]).all())
    assert res[0][1] != 0 and res[0][2] != 0  # the poisoned rows do raise the flag
    for cap in (1, 2, 4):
        assert torch.equal(res[cap][0].view(torch.int32), ref.view(torch.int32)), cap
        assert res[cap][1:] == res[0][1:], cap
    # clean data: the flag stays clear, capped or not
    for cap in (0, 2):
        ob, out = _padded(None)
        with ops.ffn_wg_cap(cap):
            launch(_padded(ffn_data["x"] if kind == "ffn" else xattn_data["x"][:M])[1], out)
        assert _flag(ops) == 0, cap


# --------------------------------------------------------------------------------------------------------------- whole clip
_CHILD = r"""
import os, sys
import numpy as np, torch
root, out = sys.argv[1:3]
sys.path[:0] = [root, os.path.join(root, "tests")]
import argparse
from tce_rvos_amd import build_model, load_synth_weights, pipeline
from _util import load_npz, synth_frames
fx = load_npz("e2e_swin_t_small.npz")
T, H, W = (int(v) for v in fx["thw"])
m, _, _ = build_model(argparse.Namespace(backbone="swin_t_p4w7", with_box_refine=True, binary=True, freeze_text_encoder=True, f_token=8,
                                         qtrans=True, num_feature_levels=4, text_encoder_layers=1))
m = m.cuda().eval()
load_synth_weights(m, int(fx["weights_salt"]))
frames = synth_frames(T, H, W, int(fx["frames_seed"])).cuda()
hid, pooled = torch.from_numpy(fx["text_hidden"])[0].cuda(), torch.from_numpy(fx["text_pooled"])[0].cuda()
keep = lambda o: {k: v.detach().cpu().numpy().copy() for k, v in o.items() if torch.is_tensor(v) and (k.startswith("pred_") or k == "memory")}
eager = keep(m.forward_features(frames, hid, pooled, float(H), float(W)))
replay = keep(m.forward_features(frames, hid, pooled, float(H), float(W)))
torch.cuda.synchronize()
assert m._graphs, "the second forward was not a graph replay"
same = all(np.array_equal(eager[k].view(np.int32), replay[k].view(np.int32)) for k in eager)
ids = torch.randint(3, 50000, (1, 9), generator=torch.Generator().manual_seed(3)).cuda()
rep = m.hazard_check(frames, ids, (H, W))
np.savez(out, eager_equals_replay=same, clean=rep.clean, report=str(rep), lat1_at=str(pipeline.LAT1_AT), lat1_cus=str(pipeline.LAT1_CUS), **eager)
"""


def _clip_child(tmp, tag, start, cap):
    env = dict(os.environ)
    env.pop("TCE_LAT1_AT", None)
    if start is not None:
        env["TCE_LAT1_AT"] = start
    env["TCE_LAT1_CUS"] = str(cap)
    # the 1350 stride-4 rows of the small clip (11 blocks) through the fused forms the cap applies to, in every child alike
    env["TCE_FFN_FUSED_MIN_ROWS"] = env["TCE_XATTN_MIN_ROWS"] = "256"
    out = os.path.join(str(tmp), tag + ".npz")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(out)


@pytest.fixture(scope="module")
def clip_uncapped(tmp_path_factory):
    return _clip_child(tmp_path_factory.mktemp("lat1"), "cap0", None, 0)


@gpu
@pytest.mark.parametrize("start", ["text", "backbone", "enc0", "enc1", "enc2"])
def test_whole_clip_capped_branch_is_bit_identical(clip_uncapped, tmp_path, start):
    """The small e2e clip with TCE_LAT1_CUS = 2 and the stride-4 branch started at each TCE_LAT1_AT option, each program in a process
    of its own (the switches are read at import): pred_* and memory are the bits of the uncapped default program, the eager pass
    equals the replayed graph, and the recorded launch program has no unordered conflicting pair."""
    ref = clip_uncapped
    assert bool(ref["clean"]) and bool(ref["eager_equals_replay"]) and str(ref["lat1_cus"]) == "0"
    got = _clip_child(tmp_path, start, start, 2)
    assert str(got["lat1_at"]) == start and str(got["lat1_cus"]) == "2"
    assert bool(got["eager_equals_replay"])
    assert bool(got["clean"]), str(got["report"])
    keys = [k for k in ref.files if k.startswith("pred_") or k == "memory"]
    assert "memory" in keys and "pred_masks" in keys and "pred_logits" in keys and "pred_boxes" in keys
    for k in keys:
        assert np.array_equal(got[k].view(np.int32), ref[k].view(np.int32)), k
