"""GPU: every kernel of csrc/text.hip (embed_ln, mha_small<64,128> behind its four entry points, caption_lens, tanh) against the fp64
references of tests/_text.py, element by element, under the bounds derived there (not calibrated on what the kernels return, no margin
added).  tests/test_text_kernels_cpu.py shows that an fp32 evaluation in the kernels' order of operations is inside the bounds on these
inputs and that each defect of _text.MUTANTS is >= 4 x outside on one of them.

Every output buffer is pre-filled with NaN (integers: a magic value) and followed by _text.GUARD sentinel rows: every element a kernel
owns must come back finite and inside its bound, and the sentinel rows untouched -- the idle queries of a last block at L = 33, 65 and
the tails of the other kernels' last workgroups store nothing.  Every case appends (entry point, case, family, max err / B,
max err / sum|terms|) to a table the last test writes to profiles/r18_text_kernels.txt."""
import os

import pytest
import torch

import _text as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r18_text_kernels.txt")
RESULTS = []
MAGIC = {torch.int32: -7, torch.uint8: 0x5A}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tce_rvos_amd import ops as _ops
    return _ops


@pytest.fixture
def lib():
    from tce_rvos_amd._lib import lib as _lib
    return _lib()


def dev(t):
    return None if t is None else t.cuda().contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def guarded(rows, *rest, dtype=torch.float32):
    """[rows + GUARD, ...] filled with NaN (integers: a magic value); the kernel gets the base pointer and owns the first `rows`."""
    fill = float("nan") if dtype.is_floating_point else MAGIC[dtype]
    return torch.full((rows + K.GUARD,) + tuple(rest), fill, dtype=dtype, device="cuda")


def sync():
    """A device error ends the session: nothing more is launched on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except Exception as e:     # noqa: BLE001
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def call(lib, name, *args):
    from tce_rvos_amd._lib import check
    check(getattr(lib, name)(*args, None), name)


# ---------------------------------------------------------------------------------------------------------------------
# one launch per case
# ---------------------------------------------------------------------------------------------------------------------
def run_mha(lib, c, entry=None, planes=None, L=None, lens=None):
    """The case through its entry point (or through `entry`, on `planes` [splits, nseq' * L, 3E] if given).  Returns the whole guarded
    buffer [nseq' * L + GUARD, E]."""
    entry = entry or c["entry"]
    planes = dev(c["planes"] if planes is None else planes)
    L = L or c["L"]
    H, splits, scale = c["nheads"], planes.shape[0], c["scale"]
    nseq = planes.shape[1] // L
    assert planes.shape[1] == nseq * L and planes.shape[2] == 3 * H * K.HD and 1 <= L <= 128 and 1 <= splits <= 64 and 1 <= nseq <= 64
    bias = dev(c["bias"])
    out = guarded(nseq * L, H * K.HD)
    if entry == "plain":
        assert splits == 1 and bias is None and nseq == 1
        call(lib, "tce_mha_small64_f32", ptr(planes), ptr(out), L, H, scale)
    elif entry == "splits":
        assert nseq == 1
        call(lib, "tce_mha_small64_splits_f32", ptr(planes), splits, ptr(bias), ptr(out), L, H, scale)
    elif entry == "seqs":
        call(lib, "tce_mha_small64_seqs_f32", ptr(planes), splits, ptr(bias), ptr(out), nseq, L, H, scale)
    else:
        assert entry == "lens"
        lt = torch.tensor(c["lens"] if lens is None else lens, dtype=torch.int32).cuda()
        assert lt.numel() == nseq
        call(lib, "tce_mha_small64_lens_f32", ptr(planes), splits, ptr(bias), ptr(out), nseq, L, H, scale, ptr(lt))
    sync()
    return out


def run_embed(lib, c):
    ids, n, C = dev(c["ids"]), c["ids"].numel(), c["C"]
    npos, vocab = c["pos"].shape[0], c["word"].shape[0]
    pid = c["pos_ids"] if c["pos_ids"] is not None else K.position_ids(c["ids"], c["pad"])
    assert C % 4 == 0 and 0 <= int(c["ids"].min()) and int(c["ids"].max()) < vocab and 0 <= int(pid.min()) and int(pid.max()) < npos
    tabs = [dev(c[k]) for k in ("word", "pos", "type0", "gamma", "beta")]
    out = guarded(n, C)
    if c["entry"] == "single":
        pos_ids = dev(c["pos_ids"])
        call(lib, "tce_embed_ln_f32", ptr(ids), ptr(pos_ids), *map(ptr, tabs), ptr(out), n, C, c["eps"], c["pad"])
    else:
        call(lib, "tce_embed_ln_seqs_f32", ptr(ids), *map(ptr, tabs), ptr(out), c["nseq"], c["seq_len"], C, c["eps"], c["pad"])
    sync()
    return out


def run_lens(ops, c):
    """ops.caption_lens with an allocator that hands out the owned part of guarded buffers; returns the three whole buffers."""
    bufs = []

    def alloc(*shape, dtype=torch.float32):
        bufs.append(guarded(*shape, dtype=dtype))
        return bufs[-1][:shape[0]]
    ops.caption_lens(dev(c["ids"]), c["pad"], alloc, D=c["D"])
    sync()
    return [b.cpu() for b in bufs]


def run_tanh(lib, x, inplace):
    n = x.numel()
    out = guarded(n)
    if inplace:
        out[:n] = x.cuda()
        src = out
    else:
        src = dev(x)
    call(lib, "tce_tanh_f32", ptr(src), ptr(out), n)
    sync()
    return out.cpu()


def record(c, r, err, S):
    rel = float((err / S)[S > 0].max()) if bool((S > 0).any()) else 0.0
    entry = {"mha": "tce_mha_small64", "embed": "tce_embed_ln", "lens": "tce_caption_lens", "tanh": "tce_tanh"}[c["kind"]]
    if c["kind"] in ("mha", "embed"):
        entry += {"plain": "_f32", "splits": "_splits_f32", "seqs": "_seqs_f32", "lens": "_lens_f32", "single": "_f32"}[c["entry"]]
    else:
        entry += "_f32"
    print(f"{entry} | {c['name']} | {c['family']} | err/B {r:.3f} | err/sum|terms| {rel:.2e}")
    RESULTS.append((entry, c["name"], c["kind"], c["family"], r, rel))


def names(kind):
    return [n for n in K.SETS if n.split(":")[0].split(" ")[0] == kind]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("mha"))
def test_mha_small_inside_the_bound(lib, name):
    c, (ref, B, S) = K.case(name)
    out = run_mha(lib, c).cpu()
    n = ref.shape[0]
    r, i = K.worst_rows(out, ref, B)
    record(c, r, (out[:n].double() - ref).abs().nan_to_num(nan=float("inf")), S)
    assert bool(torch.isnan(out[n:]).all()), f"{name}: sentinel rows written"
    assert bool(torch.isfinite(out[:n]).all()), f"{name}: {int((~torch.isfinite(out[:n])).sum())} elements not finite"
    assert r <= 1.0, f"{name}: worst err / B = {r:.3g} at row {i // ref.shape[1]}, column {i % ref.shape[1]}"


@pytest.mark.parametrize("name", names("embed"))
def test_embed_ln_inside_the_bound(lib, name):
    c, (ref, B, S) = K.case(name)
    out = run_embed(lib, c).cpu()
    n = ref.shape[0]
    r, i = K.worst_rows(out, ref, B)
    record(c, r, (out[:n].double() - ref).abs().nan_to_num(nan=float("inf")), S)
    assert bool(torch.isnan(out[n:]).all()), f"{name}: sentinel rows written"
    assert r <= 1.0, f"{name}: worst err / B = {r:.3g} at token {i // c['C']}, channel {i % c['C']}"


@pytest.mark.parametrize("name", names("lens"))
def test_caption_lens_inside_the_bound(ops, name):
    c, want = K.case(name)
    rl, rk, rp, B, S = want
    lens, kmask, pos = run_lens(ops, c)
    G, n = len(rl), rp.shape[0]
    assert lens[:G].tolist() == rl, (name, lens[:G].tolist(), rl)
    assert torch.equal(kmask[:G] != 0, rk), name
    assert bool((lens[G:] == MAGIC[torch.int32]).all() and (kmask[G:] == MAGIC[torch.uint8]).all() and torch.isnan(pos[n:]).all()), \
        f"{name}: sentinel rows written"
    r, i = K.worst_lens((lens[:G], kmask[:G], pos[:n]), want)
    record(c, r, (pos[:n].double() - rp).abs().nan_to_num(nan=float("inf")), S)
    assert r <= 1.0, f"{name}: worst err / B = {r:.3g} at row {i // c['D']}, channel {i % c['D']}"


@pytest.mark.parametrize("name", names("tanh"))
def test_tanh_inside_the_bound_and_exact_where_it_must_be(lib, name):
    c, (ref, B, S) = K.case(name)
    x, n = c["x"], c["x"].numel()
    out = run_tanh(lib, x, c["inplace"])
    ulps = K.tanh_ulp_error(out[:n], x)
    r = float(ulps.max()) / K.tanh_ulp_bound()
    record(c, r, (out[:n].double() - ref).abs().nan_to_num(nan=float("inf")), S)
    assert bool(torch.isnan(out[n:]).all()), f"{name}: sentinel elements written"
    assert r <= 1.0, f"{name}: {float(ulps.max()):.3g} ulp at x = {float(x[int(ulps.argmax())])!r}, bound {K.tanh_ulp_bound():.3g} ulp"
    assert bool((out[:n].abs() <= 1.0).all())
    inf, zero = torch.isinf(x), x == 0
    assert torch.equal(out[:n][inf], torch.sign(x[inf]))
    assert bool((out[:n][zero] == 0).all()) and torch.equal(torch.signbit(out[:n][zero]), torch.signbit(x[zero]))
    neg = run_tanh(lib, -x, c["inplace"])
    assert torch.equal(neg[:n].view(torch.int32), (-out[:n]).view(torch.int32)), f"{name}: tanh(-x) != -tanh(x) in some bit"


# ---------------------------------------------------------------------------------------------------------------------
# bit identities the code promises (same loop, same order)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mha seqs: wide, H 2 L 33 nseq 2 splits 3 +bias scale 0.1",
                                  "mha seqs: dom_last, H 2 L 31 nseq 5 splits 3 +bias scale 0.125",
                                  "mha seqs: ascending, H 2 L 33 nseq 2 splits 64 +bias scale 0.125"])
def test_seqs_is_splits_on_each_sequence_alone(lib, name):
    c, _ = K.case(name)
    L, nseq = c["L"], c["nseq"]
    out = run_mha(lib, c)
    for z in range(nseq):
        alone = run_mha(lib, c, entry="splits", planes=c["planes"][:, z * L:(z + 1) * L], L=L)
        assert torch.equal(out[z * L:(z + 1) * L], alone[:L]), (name, z)


@pytest.mark.parametrize("name", [n for n in names("mha") if n.startswith("mha plain")])
def test_one_plane_without_bias_is_the_plain_entry(lib, name):
    c, _ = K.case(name)
    plain = run_mha(lib, c)
    assert torch.equal(plain[:c["L"]], run_mha(lib, c, entry="splits")[:c["L"]]), name
    assert torch.equal(plain[:c["L"]], run_mha(lib, c, entry="seqs")[:c["L"]]), name


@pytest.mark.parametrize("name", ["mha seqs: wide, H 2 L 33 nseq 2 splits 3 +bias scale 0.1",
                                  "mha seqs: descending, H 1 L 127 nseq 2 splits 1 scale 0.125",
                                  "mha seqs: wide, H 2 L 33 nseq 2 splits 64 scale 0.1"])
def test_full_lengths_is_the_seqs_entry(lib, name):
    c, _ = K.case(name)
    n = c["nseq"] * c["L"]
    assert torch.equal(run_mha(lib, c)[:n], run_mha(lib, c, entry="lens", lens=[c["L"]] * c["nseq"])[:n]), name


# ---------------------------------------------------------------------------------------------------------------------
def test_zz_write_profile():
    """Writes the table of every case above (run the whole module: each test appends its lines)."""
    need = {("mha", f) for f in K.MHA_FAMILIES} | {("embed", f) for f in ("right", "inside", "allpad", "nopad", "right +pos_ids", "inside +pos_ids")} \
        | {("lens", "right-padded"), ("lens", "interior pad"), ("tanh", "in place"), ("tanh", "out of place")}
    seen = {(r[2], r[3]) for r in RESULTS}
    assert need <= seen, f"families that did not run: {sorted(need - seen)}"
    entries = {"tce_mha_small64_f32", "tce_mha_small64_splits_f32", "tce_mha_small64_seqs_f32", "tce_mha_small64_lens_f32",
               "tce_embed_ln_f32", "tce_embed_ln_seqs_f32", "tce_caption_lens_f32", "tce_tanh_f32"}
    assert entries <= {r[0] for r in RESULTS}, f"entry points that did not run: {sorted(entries - {r[0] for r in RESULTS})}"
    assert len({(r[0], r[1]) for r in RESULTS}) == len(K.SETS), "run the whole module"
    worst = {}
    for entry, name, kind, fam, r, rel in RESULTS:
        w = worst.setdefault((entry, fam), [0.0, 0.0, 0])
        w[0], w[1], w[2] = max(w[0], r), max(w[1], rel), w[2] + 1
    with open(PROFILE, "w") as fh:
        fh.write("# tests/test_text_kernels_gpu.py on an MI355X: per (entry point, input family) the worst case, then per case, the largest\n"
                 "# |out - fp64 ref| over the output as a fraction of the derived bound B (tests/_text.py) and of sum|terms|\n"
                 "# (mha: sum_j w_j |v_j|; embed: |gamma zhat| + |beta|; lens: |angle| + |value|; tanh: |value|).\n"
                 f"# tanh: B is {K.tanh_ulp_bound():.4g} ulp of the fp64 result = 2 x the worst error of the host's fp32 tanh against fp64 on the\n"
                 "# same grids (the ROCm installation states no bound for the device library's tanhf).\n"
                 "# entry point | family | cases | worst err/B | worst err/sum|terms|\n")
        for (entry, fam) in sorted(worst):
            w = worst[(entry, fam)]
            fh.write(f"{entry} | {fam} | {w[2]} | {w[0]:.3f} | {w[1]:.2e}\n")
        fh.write("# entry point | case | family | err/B | err/sum|terms|\n")
        for entry, name, kind, fam, r, rel in sorted(set(RESULTS)):
            fh.write(f"{entry} | {name} | {fam} | {r:.3f} | {rel:.2e}\n")
    assert all(w[0] <= 1.0 for w in worst.values())
