"""The text-encoder kernels of csrc/text.hip (embed_ln, mha_small<64,128> behind its four entry points, caption_lens, tanh): fp64
references, derived per-element bounds, a torch emulation of each kernel's order of operations, and deliberate defects.

Pure torch on the CPU; imports tests/_arith.py only.  A *case* is a dict of the tensors an entry point receives; `ref_and_bound(case)`
returns the fp64 result computed from exactly those numbers, the bound B and the natural scale S = sum |terms| of every output element.
Nothing here is fitted to what a kernel returns.  eps = 2^-24; every composed bound is first order, times 2 for the remainder as
everywhere in _arith.py, and carries no other margin.

mha_small (exact fp32, no fp16 split anywhere)
----------------------------------------------
out[i, d] = sum_j w_ij v_jd,  w = softmax_j(scale q_i . k_j),  j < Lk = clamp(lens[z], 1, L); q, k, v = sum of the partial planes + bias.

Operands.  ld4 adds `splits - 1` planes and the bias one after the other: dX = eps * splits * (sum_s |plane_s| + |bias|); zero for
one plane without bias (the load is exact).

Scores.  q * scale rounds once; each lane's quarter dot is a chain of 16 FMAs and the two shuffle adds join the quarters: c = 18 + 1
roundings against |scale| sum_d |q_d| |k_d|.  The operand errors chain through the product: |scale| (dq |k|^T + |q| dk^T).  The
subtraction of the running maximum and the base-2 conversion inside __expf: eps (|s| + 2 |s - max|).  The exponents of one key telescope
along the keys: p_j is taken against the running maximum and rescaled by corr = exp(m_old - m_new) at every later change of it; all the
differences have one sign, so their magnitudes add up to |s_j - max| exactly and the term is counted once.
    Bs_ij = eps (19 |scale| sum |q||k| + |s_ij| + 2 |s_ij - max_i|) + |scale| (dq |k|^T + |q| dk^T)_ij

The hardware exponential.  Its accuracy is the one number the code does not give, and the kernel / micro-architecture guides this
project follows do not state one either; it is MODELLED here as EXP_ULPS = 2 ulp of p (relative 2 * 2^-23).  Key j's weight carries its
own exponential and at most Lk - 1 corr factors (a corr of exp(0) = 1 is exact): (EXP_ULPS * 2 eps) * Lk.  Both are common to the
numerator o and the denominator l, as is Bs, so they act on |v_jd - out_d|:
    rc_ij = Bs_ij + EXP_ULPS * 2 eps * Lk

Key-by-key accumulation (read off the loop).  Per key, o takes one product o * corr and one FMA, l one product and one add: a term
that entered at key j meets 2 roundings at each of at most Lk keys, separately in o and in l: ri = 2 eps Lk on sum_j w_j |v_jd| and
on |out_d|.  A weight below the normal range (exp(-100)) is lost or denormal: 2^-126 sum_j |v_jd|.

Final reciprocal and product: 1 / l is one correctly rounded division (the build has no fast-math flag), o * inv one product: 2 eps |out|.

    B = 2 [ sum_j w_j rc_ij |v_jd - out_d| + ri (sum_j w_j |v_jd| + |out_d|) + sum_j w_j dv_jd + 2 eps |out_d| + 2^-126 sum_j |v_jd| ]

embed_ln
--------
z = (word + type0) + pos is two fp32 adds: Bz = 2 eps (|w| + |t| + |p|); then A.ln_tail.  B = 2 ln_tail(z, Bz).  The inputs must have
layernorm_sigma(z) > 1e-3 on every row (asserted in ref_and_bound: a condition on the inputs, as in the arithmetic suite).

caption_lens
------------
lens and the key mask are integers: exact.  pos = sin | cos (a), a = x / dim_t, x = min(j + 1, n) / (n + 1e-6) * 2 pi,
dim_t = 10000 ^ e, e = 2 (c / 2) / D.  x: the add of 1e-6, the division, the product and fp32's 2 pi: 4 eps; the division by dim_t: 1;
e is one rounded division, which moves dim_t by ln(10000) e eps; powf itself is modelled at POW_ULPS = 2 ulp (exact at e = 0):
    da = eps |a| (5 + ln(10000) e + 4 [e > 0])
sinf / cosf have slope <= 1 and are modelled at SINCOS_ULPS = 2 ulp of the result: B = min(2 (da + 4 eps |y|), 2e-6) -- never looser
than the 2e-6 the suite held this table to before.

tanh
----
In ulp of the fp64 result (ulp of the fp32 binade it falls in).  The ROCm installation documents no bound for the device library's
tanhf, so the bound is 2 x the worst error torch.tanh in fp32 on the CPU shows against fp64 on the same grid (tanh_ulp_bound).

Defects.  MHA_MUTANTS / EMBED_MUTANTS / LENS_MUTANTS are keywords of emulate().  "query_mod_L" needs a remark: replacing the idle
queries' row min(i, L - 1) by i % L changes no stored value as long as the store guard `i >= L` is intact, so the defect is modelled
as the wrapped query being stored at row i, which lands on the next sequence's rows or on the sentinel rows after the buffer;
emulate() therefore returns GUARD extra rows that a correct kernel leaves untouched (NaN), and worst_rows() counts a touched one as
infinitely wrong.

Corrections of the derivation made after a correct evaluation exceeded B: none."""
import math

import torch

import _arith as A

F64 = torch.float64
F32 = torch.float32
EPS = A.EPS_F32
HD = 64            # head width
GUARD = 32         # sentinel rows after every output buffer
EXP_ULPS = 2.0     # modelled accuracy of the hardware exponential, ulp of p
POW_ULPS = 2.0
SINCOS_ULPS = 2.0

MHA_MUTANTS = ("o_no_corr", "l_no_corr", "scale_twice", "keys_plus_1", "keys_minus_1", "lens_prev_seq", "lens_no_clamp",
               "stride_no_nseq", "drop_last_plane", "bias_per_plane", "bias_off_v", "kv_swapped", "head_off_32", "query_mod_L",
               "shuffle_one_step")
EMBED_MUTANTS = ("count_no_restart", "count_excludes_current", "pad_gets_count", "lanes_ge64_not_counted", "pad_id_fixed_1",
                 "no_type0", "var_over_c_minus_1", "no_eps", "pos_ids_ignored")
LENS_MUTANTS = ("last_pad", "lens_zero_allowed", "no_min")
MUTANTS = {"mha": MHA_MUTANTS, "embed": EMBED_MUTANTS, "lens": LENS_MUTANTS, "tanh": ()}

MHA_FAMILIES = ("uniform", "wide", "ascending", "descending", "identical", "dom_first", "dom_last", "dom_lkm1", "offset")


def _d(x):
    return x.detach().to("cpu", F64)


# =====================================================================================================================
# mha_small
# =====================================================================================================================
def clamp_len(n, L):
    return min(max(int(n), 1), L)


def mha_case(family, nheads, L, nseq=1, splits=1, bias=False, scale=0.125, entry=None, lens=None, seed=0):
    """planes [splits, nseq * L, 3E] fp32 whose sum (+ bias) has the family's score structure.  entry: the entry point that runs it
    ("plain", "splits", "seqs", "lens"); lens: one int per sequence (values outside 1..L are the clamp), K / V rows >= clamp(lens) are
    NaN in every plane and Q stays finite."""
    E = nheads * HD
    if entry is None:
        entry = "lens" if lens is not None else "seqs" if nseq > 1 else "splits" if (splits > 1 or bias) else "plain"
    assert entry != "plain" or (nseq == 1 and splits == 1 and not bias and lens is None)
    assert entry != "splits" or (nseq == 1 and lens is None)
    assert (entry == "lens") == (lens is not None)
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    q, k, v = rn(nseq, nheads, L, HD), rn(nseq, nheads, L, HD), rn(nseq, nheads, L, HD)
    lk = [clamp_len(n, L) for n in lens] if lens is not None else [L] * nseq
    sig = math.sqrt(0.3 / (8.0 * abs(scale)))     # logits of std 0.3
    if family == "wide":
        q, k = 3.0 * q, 3.0 * k
    elif family in ("ascending", "descending", "identical"):
        u = rn(nseq, nheads, 1, HD)
        u = u / u.norm(dim=-1, keepdim=True) / math.sqrt(abs(scale))          # scale |u|^2 = 1
        a = 0.5 + torch.rand(nseq, nheads, L, 1, generator=g, dtype=F64)
        t = 0.25 * torch.arange(L, dtype=F64) + 0.1 * torch.rand(L, generator=g, dtype=F64)
        if family == "descending":
            t = t.flip(0)
        if family == "identical":
            t = torch.full((L,), 3.0, dtype=F64)
        q, k = a * u, t.view(1, 1, L, 1) * u
        if scale < 0:
            k = -k
    else:
        q, k = sig * q, sig * k
        if family.startswith("dom_"):
            q[..., 0] = 4.0
            for z in range(nseq):
                j = {"dom_first": 0, "dom_last": L - 1, "dom_lkm1": lk[z] - 1}[family]
                k[z, :, j, 0] = 30.0 / (scale * 4.0)
        elif family == "offset":
            q[..., 1] = 40.0
            k[..., 1] = -200.0 / (scale * 40.0)
        else:
            assert family == "uniform", family
    x = torch.cat([t.permute(0, 2, 1, 3).reshape(nseq * L, E) for t in (q, k, v)], dim=1).float()     # [nseq L, 3E]
    b = (0.5 * torch.randn(3 * E, generator=g)).float() if bias else None
    planes = torch.empty(splits, nseq * L, 3 * E)
    for s in range(splits - 1):
        planes[s] = x / splits + 0.05 * torch.randn(nseq * L, 3 * E, generator=g)
    rest = x - (b if bias else 0.0)
    for s in range(splits - 1):
        rest = rest - planes[s]
    planes[splits - 1] = rest
    if lens is not None:
        for z in range(nseq):
            planes[:, z * L + lk[z]:(z + 1) * L, E:] = float("nan")
    name = f"{family}, H {nheads} L {L} nseq {nseq} splits {splits}{' +bias' if bias else ''} scale {scale:g}"
    if lens is not None:
        name += f" lens {tuple(lens)}"
    return dict(kind="mha", family=family, name=name, entry=entry, planes=planes, bias=b, L=L, nseq=nseq, nheads=nheads,
                splits=splits, scale=float(scale), lens=None if lens is None else [int(n) for n in lens])


def _heads(x, nheads):
    """[rows, nheads * 64] -> [nheads, rows, 64]"""
    return x.view(x.shape[0], nheads, HD).permute(1, 0, 2)


def mha_ref_and_bound(c):
    """(ref, B, S), each [nseq * L, E] fp64."""
    L, nseq, H, splits, scale = c["L"], c["nseq"], c["nheads"], c["splits"], c["scale"]
    E = H * HD
    sc = abs(scale)
    bias = None if c["bias"] is None else _d(c["bias"])
    P = _d(c["planes"])
    ref, B, S = (torch.empty(nseq * L, E, dtype=F64) for _ in range(3))
    for z in range(nseq):
        Lk = clamp_len(c["lens"][z], L) if c["lens"] is not None else L
        X = P[:, z * L:(z + 1) * L]
        x, ax = X.sum(0), X.abs().sum(0)
        if bias is not None:
            x, ax = x + bias, ax + bias.abs()
        dx = EPS * splits * ax if (splits > 1 or bias is not None) else torch.zeros_like(ax)
        q, dq = _heads(x[:, :E], H), _heads(dx[:, :E], H)
        k, dk = _heads(x[:Lk, E:2 * E], H), _heads(dx[:Lk, E:2 * E], H)
        v, dv = _heads(x[:Lk, 2 * E:], H), _heads(dx[:Lk, 2 * E:], H)
        assert bool(torch.isfinite(q).all() and torch.isfinite(k).all() and torch.isfinite(v).all())
        for h in range(H):
            s = scale * (q[h] @ k[h].T)                                         # [L, Lk]
            smax = s.max(dim=1, keepdim=True).values
            Bs = EPS * (19.0 * sc * (q[h].abs() @ k[h].abs().T) + s.abs() + 2.0 * (s - smax).abs()) \
                + sc * (dq[h] @ k[h].abs().T + q[h].abs() @ dk[h].T)
            rc = Bs + EXP_ULPS * 2.0 * EPS * Lk
            ri = 2.0 * EPS * Lk
            w = torch.softmax(s, dim=1)
            out = w @ v[h]                                                      # [L, 64]
            Sv = w @ v[h].abs()
            spread = torch.einsum("ij,ijd->id", w * rc, (v[h][None, :, :] - out[:, None, :]).abs())
            b = spread + ri * (Sv + out.abs()) + w @ dv[h] + 2.0 * EPS * out.abs() + 2.0 ** -126 * v[h].abs().sum(0, keepdim=True)
            rows, cols = slice(z * L, (z + 1) * L), slice(h * HD, (h + 1) * HD)
            ref[rows, cols], B[rows, cols], S[rows, cols] = out, 2.0 * b, Sv
    return ref, B, S


def emulate_mha(c, dt=F64, mutant=None):
    """The kernel's order of operations in torch at precision dt: planes summed one after the other, then the bias; q * scale; four
    quarter dots of 16 sequential multiply-adds joined by two exchange steps; keys one at a time with the running maximum starting at
    -3e38, l and o rescaled by corr at every key; o * (1 / l).  Returns [nseq * L + GUARD, E]; rows no query stores stay NaN."""
    assert mutant is None or mutant in MHA_MUTANTS, mutant
    L, nseq, H, splits, scale = c["L"], c["nseq"], c["nheads"], c["splits"], c["scale"]
    E = H * HD
    flat = c["planes"].to(dt).reshape(splits * nseq * L, 3 * E)
    bias = None if c["bias"] is None else c["bias"].to(dt)
    pstride = L if mutant == "stride_no_nseq" else nseq * L
    nplanes = splits - 1 if (mutant == "drop_last_plane" and splits > 1) else splits
    out = torch.full((nseq * L + GUARD, E), float("nan"), dtype=dt)
    hcol = 32 if mutant == "head_off_32" else HD
    for z in range(nseq):
        if c["lens"] is None:
            Lk = L
        else:
            n = c["lens"][(z - 1) % nseq] if mutant == "lens_prev_seq" else c["lens"][z]
            Lk = min(n, L) if mutant == "lens_no_clamp" else clamp_len(n, L)
        nk = Lk + 1 if mutant == "keys_plus_1" else Lk - 1 if mutant == "keys_minus_1" else Lk
        nk = max(nk, 0)
        rows = torch.arange(max(L, nk))
        x = None
        for s in range(nplanes):
            idx = (s * pstride + z * L + rows).clamp(max=flat.shape[0] - 1)     # a key past the buffer: the last row again
            x = flat[idx] if x is None else x + flat[idx]
        if bias is not None:
            b = bias.clone()
            if mutant == "bias_off_v":
                b[2 * E:] = 0
            for _ in range(splits if mutant == "bias_per_plane" else 1):
                x = x + b
        cols = (torch.arange(H) * hcol)[:, None] + torch.arange(HD)[None, :]      # [H, 64]
        q = x[:L][:, cols].permute(1, 0, 2)                                       # [H, L, 64]
        k = x[:nk][:, E + cols].permute(1, 0, 2)
        v = x[:nk][:, 2 * E + cols].permute(1, 0, 2)
        if mutant == "kv_swapped":
            k, v = v, k
        q = q * scale
        if mutant == "scale_twice":
            q = q * scale
        qq, kk = q.reshape(H, L, 1, 4, 16), k.reshape(H, 1, nk, 4, 16)
        a = torch.zeros(H, L, nk, 4, dtype=dt)
        for d in range(16):
            a = a + qq[..., d] * kk[..., d]
        a = a + a[..., [1, 0, 3, 2]]
        if mutant != "shuffle_one_step":
            a = a + a[..., [2, 3, 0, 1]]
        m = torch.full((H, L, 4), -3.0e38, dtype=dt)
        l = torch.zeros(H, L, 4, dtype=dt)
        o = torch.zeros(H, L, 4, 16, dtype=dt)
        vv = v.reshape(H, nk, 4, 16)
        for j in range(nk):
            aj = a[:, :, j]
            mnew = torch.maximum(m, aj)
            corr, pj = torch.exp(m - mnew), torch.exp(aj - mnew)
            l = (l if mutant == "l_no_corr" else l * corr) + pj
            o = pj[..., None] * vv[:, None, j] + (o if mutant == "o_no_corr" else o * corr[..., None])
            m = mnew
        res = (o * (1.0 / l)[..., None]).reshape(H, L, HD).permute(1, 0, 2).reshape(L, E)
        out[z * L:(z + 1) * L] = res
        if mutant == "query_mod_L":
            for i in range(L, -(-L // 32) * 32):
                out[z * L + i] = res[i % L]
    return out


def worst_rows(out, ref, B):
    """A.worst on the rows of ref; every further row of `out` is a sentinel row and must still be NaN."""
    n = ref.shape[0]
    r, i = A.worst(out[:n], ref, B)
    if out.shape[0] > n and not bool(torch.isnan(out[n:]).all()):
        return float("inf"), n * ref.shape[1]
    return r, i


# =====================================================================================================================
# embed_ln
# =====================================================================================================================
def embed_ids(nseq, seq_len, pad, pattern, vocab=64, seed=0):
    """pattern: "right" (right-padded, one caption full), "inside" (pads between tokens), "allpad" (first caption all pad), "nopad"."""
    g = torch.Generator().manual_seed(2000 + seed)
    ids = torch.randint(0, vocab, (nseq, seq_len), generator=g)
    ids[ids == pad] = (pad + 1) % vocab
    for z in range(nseq):
        if pattern == "right":
            n = seq_len if z == nseq - 1 and nseq > 1 else max(1, (seq_len * (z + 2)) // (nseq + 2))
            ids[z, n:] = pad
        elif pattern == "inside":
            ids[z, torch.rand(seq_len, generator=g) < 0.3] = pad
            if seq_len > 2:
                ids[z, 1], ids[z, 2] = pad, (pad + 1) % vocab
        elif pattern == "allpad" and z == 0:
            ids[z] = pad
    return ids


def embed_case(C, nseq, seq_len, pad=1, pattern="right", given_pos=False, entry=None, seed=0, vocab=64):
    """Random tables of std 0.02 (the scale of the model's own): vocab rows of words, pad + seq_len + 2 rows of positions."""
    assert C % 4 == 0
    entry = entry or ("single" if nseq == 1 else "seqs")
    assert entry == "seqs" or nseq == 1
    assert not given_pos or entry == "single"
    g = torch.Generator().manual_seed(3000 + seed)
    npos = pad + seq_len + 2
    ids = embed_ids(nseq, seq_len, pad, pattern, vocab, seed)
    c = dict(kind="embed", family=pattern + (" +pos_ids" if given_pos else ""), entry=entry, ids=ids, pad=pad, C=C, nseq=nseq,
             seq_len=seq_len, eps=1e-5,
             word=0.02 * torch.randn(vocab, C, generator=g), pos=0.02 * torch.randn(npos, C, generator=g),
             type0=0.02 * torch.randn(C, generator=g), gamma=1.0 + 0.1 * torch.randn(C, generator=g), beta=0.1 * torch.randn(C, generator=g),
             pos_ids=torch.randint(0, npos, (1, seq_len), generator=g) if given_pos else None)
    c["name"] = f"{c['family']}, C {C} nseq {nseq} L {seq_len} pad {pad}"
    return c


def position_ids(ids, pad):
    """HF create_position_ids_from_input_ids, per caption (row)."""
    mask = (ids != pad).long()
    return pad + torch.cumsum(mask, dim=1) * mask


def embed_ref_and_bound(c):
    ids, pad, C = c["ids"], c["pad"], c["C"]
    pid = c["pos_ids"] if c["pos_ids"] is not None else position_ids(ids, pad)
    w, p, t = _d(c["word"])[ids.flatten()], _d(c["pos"])[pid.flatten()], _d(c["type0"])[None, :]
    z = w + p + t
    assert float(A.layernorm_sigma(z).min()) > 1e-3, "degenerate row: choose other inputs"
    ref = torch.nn.functional.layer_norm(z, (C,), _d(c["gamma"]), _d(c["beta"]), c["eps"])
    Bz = 2.0 * EPS * (w.abs() + t.abs() + p.abs())
    B = 2.0 * A.ln_tail(z, Bz, c["gamma"], c["beta"], c["eps"])
    S = (ref - _d(c["beta"])).abs() + _d(c["beta"]).abs()
    return ref, B, S


def _wave_sum(x):
    """[rows, 64] -> [rows]: the xor butterfly, offsets 32 .. 1."""
    o = 32
    lanes = torch.arange(64)
    while o:
        x = x + x[:, lanes ^ o]
        o >>= 1
    return x[:, 0]


def _lane_sum(x4):
    """x4 [rows, n4, 4] pre-reduced groups -> per-lane strided accumulation then the butterfly."""
    rows, n4 = x4.shape[0], x4.shape[1]
    g = (x4[..., 0] + x4[..., 1]) + (x4[..., 2] + x4[..., 3])
    acc = torch.zeros(rows, 64, dtype=x4.dtype)
    for i0 in range(0, n4, 64):
        blk = g[:, i0:i0 + 64]
        acc[:, :blk.shape[1]] = acc[:, :blk.shape[1]] + blk
    return _wave_sum(acc)


def emulate_embed(c, dt=F64, mutant=None):
    """One wavefront per token: lane-strided count of the caption's non-pad tokens up to the token (64 lanes, wave sum), (w + t) + p,
    lane-strided sums of groups of four and the butterfly for mean and variance, (v - mean) * rstd * g + b.  [nseq * seq_len + GUARD, C]."""
    assert mutant is None or mutant in EMBED_MUTANTS, mutant
    ids, C, sl = c["ids"].flatten(), c["C"], c["seq_len"]
    pad = 1 if mutant == "pad_id_fixed_1" else c["pad"]
    n = ids.numel()
    if c["pos_ids"] is not None and mutant != "pos_ids_ignored":
        pid = c["pos_ids"].flatten()
    else:
        pid = torch.empty(n, dtype=torch.int64)
        nonpad = (ids != pad).long().tolist()
        cs = [0]
        for b in nonpad:
            cs.append(cs[-1] + b)
        for tok in range(n):
            start = 0 if mutant == "count_no_restart" else (tok // sl) * sl
            # lane l counts ids[start + l], ids[start + l + 64], ... up to tok and the wave sum adds the 64 integers (exact): all of
            # start .. tok; a lane that never steps on sees its first element only
            last = min(start + 63, tok) if mutant == "lanes_ge64_not_counted" else tok
            cnt = cs[last + 1] - cs[start]
            if mutant == "count_excludes_current":
                cnt -= int(nonpad[tok])
            pid[tok] = pad + cnt if (nonpad[tok] or mutant == "pad_gets_count") else pad
    ptab = c["pos"].to(dt)
    if int(pid.max()) >= ptab.shape[0]:     # a defect that walks off the table reads whatever lies behind it
        ptab = torch.cat([ptab, torch.full((int(pid.max()) + 1 - ptab.shape[0], C), float("nan"), dtype=dt)])
    w, p, t = c["word"].to(dt)[ids], ptab[pid], c["type0"].to(dt)[None, :]
    v = (w if mutant == "no_type0" else w + t) + p
    mean = (_lane_sum(v.view(n, C // 4, 4)) / C)[:, None]
    dlt = v - mean
    var = _lane_sum((dlt * dlt).view(n, C // 4, 4)) / (C - 1 if mutant == "var_over_c_minus_1" else C)
    rstd = (1.0 / torch.sqrt(var if mutant == "no_eps" else var + torch.tensor(c["eps"], dtype=dt)))[:, None]
    out = torch.full((n + GUARD, C), float("nan"), dtype=dt)
    out[:n] = dlt * rstd * c["gamma"].to(dt) + c["beta"].to(dt)
    return out


# =====================================================================================================================
# caption_lens
# =====================================================================================================================
def lens_case(Lmax, D, lens, pad=1, interior=False, seed=0):
    """ids [G, Lmax] right-padded to lens[g] tokens; interior: a further token after the first pad of every padded caption (the first
    pad rules)."""
    g = torch.Generator().manual_seed(4000 + seed)
    ids = torch.randint(pad + 1, 60, (len(lens), Lmax), generator=g)
    for b, n in enumerate(lens):
        ids[b, n:] = pad
        if interior and n + 1 < Lmax:
            ids[b, n + 1] = pad + 7
    return dict(kind="lens", family="interior pad" if interior else "right-padded", entry="caption_lens", ids=ids, pad=pad, D=D,
                Lmax=Lmax, name=f"Lmax {Lmax} D {D} lens {tuple(lens)}{' interior' if interior else ''}")


def lens_rule(ids, pad, mutant=None):
    """lens[b]: index of the first pad id, Lmax if none, at least 1."""
    G, Lmax = ids.shape
    out = []
    for b in range(G):
        hits = (ids[b] == pad).nonzero().flatten()
        first = Lmax if hits.numel() == 0 else int(hits[-1] if mutant == "last_pad" else hits[0])
        out.append(first if mutant == "lens_zero_allowed" else max(first, 1))
    return out


def _pos_table(lens, Lmax, D, dt, mutant=None):
    tens = lambda x: torch.tensor(x, dtype=dt)
    out = []
    c = torch.arange(D)
    e = (2 * (c // 2)).to(dt) / tens(float(D))
    dim_t = torch.pow(tens(10000.0), e)
    j1 = torch.arange(1, Lmax + 1).to(dt)
    for n in lens:
        x = j1 if mutant == "no_min" else torch.clamp(j1, max=float(n))
        x = x / (tens(float(n)) + tens(1e-6)) * tens(6.28318530717958647692)
        a = x[:, None] / dim_t[None, :]
        out.append(torch.where((c % 2 == 1)[None, :], a.cos(), a.sin()))
    return torch.cat(out, 0), e


def lens_ref_and_bound(c):
    """(lens list, kmask bool [G, Lmax], pos fp64 [G * Lmax, D], B, S)."""
    ids, D, Lmax = c["ids"], c["D"], c["Lmax"]
    lens = lens_rule(ids, c["pad"])
    kmask = torch.arange(Lmax)[None, :] >= torch.tensor(lens)[:, None]
    pos, e = _pos_table(lens, Lmax, D, F64)
    j1 = torch.arange(1, Lmax + 1, dtype=F64)
    a = torch.cat([torch.clamp(j1, max=float(n)) / (n + 1e-6) * (2 * math.pi) for n in lens])[:, None] / torch.pow(torch.tensor(10000.0, dtype=F64), e)[None, :]
    da = EPS * a.abs() * (5.0 + math.log(10000.0) * e + 2.0 * POW_ULPS * (e > 0).to(F64))[None, :]
    B = torch.clamp(2.0 * (da + SINCOS_ULPS * 2.0 * EPS * pos.abs()), max=2e-6)
    return lens, kmask, pos, B, a.abs() + pos.abs()


def emulate_lens(c, dt=F64, mutant=None):
    assert mutant is None or mutant in LENS_MUTANTS, mutant
    lens = lens_rule(c["ids"], c["pad"], mutant)
    kmask = torch.arange(c["Lmax"])[None, :] >= torch.tensor(lens)[:, None]
    pos, _ = _pos_table(lens, c["Lmax"], c["D"], dt, mutant)
    return lens, kmask, pos


def worst_lens(got, want):
    """got = (lens, kmask, pos) against want = lens_ref_and_bound: a wrong integer is infinitely wrong."""
    lens, kmask, pos = got
    rl, rk, rp, B = want[:4]
    if [int(v) for v in lens] != [int(v) for v in rl] or not torch.equal(torch.as_tensor(kmask).cpu() != 0, rk):
        return float("inf"), 0
    return A.worst(pos, rp, B)


# =====================================================================================================================
# tanh
# =====================================================================================================================
TANH_SPECIAL = (0.0, -0.0, 1e-30, -1e-30, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, float("inf"), -float("inf"))


def tanh_values(n):
    """n fp32 values: the special ones first (as many as fit), then a dense grid on [-10, 10]."""
    sp = torch.tensor(TANH_SPECIAL, dtype=F32)
    if n == 1:
        return torch.tensor([0.7], dtype=F32)
    if n <= sp.numel():
        return sp[:n].clone()
    return torch.cat([sp, torch.linspace(-10.0, 10.0, n - sp.numel(), dtype=F32)])


def tanh_case(n, inplace):
    return dict(kind="tanh", family="in place" if inplace else "out of place", entry="tanh", x=tanh_values(n), inplace=inplace,
                name=f"n {n}{' in place' if inplace else ''}")


def ulp32(y):
    """Spacing of fp32 at |y| (fp64 tensor): 2^(floor(log2 |y|) - 23), 2^-149 below the normal range."""
    y = _d(y).abs()
    ex = torch.floor(torch.log2(torch.clamp(y, min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), ex - 23.0)


def tanh_ulp_error(out, x):
    """|out - tanh64(x)| in ulp of the fp64 result, per element (inf on a NaN)."""
    ref = torch.tanh(_d(x))
    return ((_d(out) - ref).abs() / ulp32(ref)).nan_to_num(nan=float("inf"))


def tanh_ulp_bound():
    """2 x the worst error of torch.tanh in fp32 on the CPU against fp64 over every grid the cases use."""
    worst = 0.0
    for n in (1, 255, 256, 257, 2304):
        x = tanh_values(n)
        worst = max(worst, float(tanh_ulp_error(torch.tanh(x), x).max()))
    return 2.0 * worst


def tanh_ref_and_bound(c):
    ref = torch.tanh(_d(c["x"]))
    return ref, tanh_ulp_bound() * ulp32(ref), ref.abs()


# =====================================================================================================================
def ref_and_bound(c):
    return {"mha": mha_ref_and_bound, "embed": embed_ref_and_bound, "tanh": tanh_ref_and_bound}[c["kind"]](c)


def emulate(c, mutant=None, dt=F64):
    """The case's kernel restated in torch, optionally with one defect (a keyword of MUTANTS[kind])."""
    if c["kind"] == "tanh":
        assert mutant is None
        return torch.tanh(c["x"].to(dt))
    return {"mha": emulate_mha, "embed": emulate_embed, "lens": emulate_lens}[c["kind"]](c, dt, mutant)


# ---- the input sets: name -> builder.  The CPU module proves the bounds discriminate on exactly these; the GPU module runs them. ----
def _mha_sets():
    s = {}

    def add(*a, **k):
        c = mha_case(*a, **k)
        s[f"mha {c['entry']}: {c['name']}"] = (lambda a=a, k=k: mha_case(*a, **k))
    # every block edge, one plane (the plain entry), alternating families so that each is met at more than one length
    for i, L in enumerate((1, 31, 32, 33, 64, 65, 127, 128)):
        add(("uniform", "wide", "ascending", "descending", "dom_last", "offset", "identical", "dom_first")[i], 1 if L > 64 else 2, L, seed=i)
    for i, fam in enumerate(MHA_FAMILIES):
        if fam != "dom_lkm1":
            add(fam, 2, 33, nseq=2, splits=3, bias=True, scale=0.1, seed=20 + i)
    add("wide", 12, 128, seed=30)
    add("wide", 12, 65, splits=3, bias=True, seed=31)
    add("uniform", 1, 32, splits=3, bias=False, scale=0.1, seed=32)
    add("ascending", 2, 33, nseq=2, splits=64, bias=True, seed=33)
    add("wide", 2, 33, nseq=2, splits=64, bias=False, scale=0.1, seed=34)
    add("dom_last", 2, 31, nseq=5, splits=3, bias=True, seed=35)
    add("descending", 1, 127, nseq=2, seed=36)
    # lens: 1, L, L/2, 32, 33, 0 and L + 5 (the clamp), NaN keys past each
    add("wide", 2, 65, nseq=5, splits=3, bias=True, scale=0.1, lens=(1, 65, 32, 33, 0), seed=40)
    add("dom_lkm1", 2, 65, nseq=5, splits=1, lens=(33, 70, 32, 1, 65), seed=41)
    add("dom_lkm1", 1, 127, nseq=2, splits=3, bias=True, lens=(63, 127), seed=42)
    add("ascending", 12, 33, nseq=2, splits=3, bias=True, lens=(0, 38), seed=43)
    add("uniform", 2, 31, nseq=5, splits=1, lens=(31, 15, 1, 36, 0), seed=44)
    add("dom_first", 1, 128, nseq=1, splits=1, lens=(64,), seed=45)
    return s


def _embed_sets():
    s = {}

    def add(*a, **k):
        c = embed_case(*a, **k)
        s[f"embed {c['entry']}: {c['name']}"] = (lambda a=a, k=k: embed_case(*a, **k))
    for i, (C, L) in enumerate(((4, 1), (252, 4), (256, 5), (260, 7), (768, 100))):
        add(C, 1, L, pad=(1, 5)[i % 2], pattern=("nopad", "right", "inside", "right", "inside")[i], seed=i)
    add(256, 1, 7, pad=5, pattern="inside", given_pos=True, seed=10)
    add(768, 1, 100, pad=1, pattern="right", given_pos=True, seed=11)
    add(260, 1, 5, pad=1, pattern="allpad", seed=12)
    for i, (nseq, L) in enumerate(((2, 11), (3, 5), (2, 70), (2, 128))):
        add((252, 4, 768, 256)[i], nseq, L, pad=(5, 1)[i % 2], pattern=("inside", "allpad", "right", "nopad")[i], seed=20 + i)
    add(260, 2, 70, pad=5, pattern="inside", seed=30)
    add(768, 3, 5, pad=1, pattern="right", seed=31)
    add(768, 1, 7, pad=1, pattern="nopad", seed=40)     # what the earlier tests ran: one un-padded caption, pad id 1
    return s


def _lens_sets():
    s = {}
    for i, (Lmax, D, lens, interior) in enumerate(((1, 2, (1,), False), (33, 2, (1, 33, 17), False), (33, 256, (33, 16, 1), True),
                                                   (128, 256, (128, 1, 64), False), (128, 2, (64, 127, 5), True), (33, 256, (0, 5), False))):
        c = lens_case(Lmax, D, lens, interior=interior, seed=i)
        s[f"lens: {c['name']}"] = (lambda a=(Lmax, D, lens), k=dict(interior=interior, seed=i): lens_case(*a, **k))
    return s


def _tanh_sets():
    return {f"tanh: {tanh_case(n, ip)['name']}": (lambda n=n, ip=ip: tanh_case(n, ip)) for n in (1, 255, 256, 257, 2304) for ip in (False, True)}


SETS = {**_mha_sets(), **_embed_sets(), **_lens_sets(), **_tanh_sets()}
NEAR_UNIFORM = {"mha": "mha seqs: uniform, H 2 L 33 nseq 2 splits 3 +bias scale 0.1", "embed": None, "lens": None}
_CACHE = {}


def case(name):
    """(case, reference tuple), built once and left unchanged."""
    if name not in _CACHE:
        c = SETS[name]()
        _CACHE[name] = (c, lens_ref_and_bound(c) if c["kind"] == "lens" else ref_and_bound(c))
    return _CACHE[name]


def ratio(c, got, want):
    """Worst err / B of a result (emulated or from the device) against case()'s reference tuple."""
    if c["kind"] == "lens":
        return worst_lens(got, want)[0]
    if c["kind"] == "tanh":
        return float((tanh_ulp_error(got, c["x"]) / tanh_ulp_bound()).max())
    return worst_rows(got, want[0], want[1])[0]
