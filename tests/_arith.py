"""Per-element error bounds of the split-fp16 matrix arithmetic, and a CPU emulation of it with deliberate defects.

Pure torch on the CPU, fp64 throughout; imports nothing of the project.  Every product of the HIP kernels is evaluated as
hi_a*hi_b + hi_a*lo_b + lo_a*hi_b on fp16 matrix cores with fp32 accumulation, under the documented operand contract
|x - hi - lo| <= max(2^-20 |x|, 2^-24).  The bounds here follow from that contract and from the number formats;
nothing in them is fitted to what a kernel returns.

Operand convention: a [M, K] activations, w [N, K] weights (nn.Linear layout), products are a @ w.T -> [M, N].
"""
import math

import torch

F64 = torch.float64
EPS_SPLIT = 2.0 ** -20     # relative residual of a two-half fp16 representation (contract)
FLOOR_SPLIT = 2.0 ** -24   # its absolute floor: the smallest fp16 subnormal (contract)
EPS_F32 = 2.0 ** -24       # unit round-off of fp32
GELU_LIPSCHITZ = 1.13      # max |d/dx GELU(x)| = 1.1289...

# Dense products: the accumulation term uses c = DENSE_C_FACTOR * sqrt(3 K) (random-sign model of 3 K fp32 additions).  The model is
# validated on the GPU against the exact-fp32 MFMA kernel (mode "f32"), never against a split kernel; if that kernel does not stay
# inside bound_acc with a factor 2 of room the factor is raised to the next power of two that gives it and recorded here.
DENSE_C_FACTOR = 1.0

# (weight scale, activation scale) grids of the GPU module; the CPU module proves the bounds discriminate on exactly these.
DENSE_SCALES = ((1.0, 1.0), (2.0 ** -4, 1.0), (2.0 ** -8, 1.0), (1.0, 2.0 ** -8), (2.0 ** 4, 2.0 ** 4))
PROBE_SCALES = ((1.0, 1.0), (2.0 ** -4, 1.0), (1.0, 2.0 ** -8))
# every K extent a GPU case multiplies over (dense) / probes by 8-wide block
DENSE_K = (16, 32, 48, 64, 96, 128, 160, 192, 256, 288, 384, 512, 576, 768, 2048, 2304, 3072, 6912)
PROBE_K = (64, 96, 128, 192, 256, 384, 512, 768, 2048, 2304, 3072)


_WHERE = ["cpu"]


class on:
    """`with A.on("cuda"):` -- the bounds inside are evaluated in fp64 on that device (the same formulas; for references whose
    per-head loop over a few thousand queries x a thousand keys x 128 heads would take the CPU seconds per case)."""

    def __init__(self, device):
        self.device, self.prev = str(device), None

    def __enter__(self):
        self.prev, _WHERE[0] = _WHERE[0], self.device
        return self

    def __exit__(self, *exc):
        _WHERE[0] = self.prev
        return False


def _d(x):
    return x.detach().to(_WHERE[0], F64)


def delta(x):
    """Contract: what hi + lo may miss of x."""
    x = _d(x).abs()
    return torch.clamp(x * EPS_SPLIT, min=FLOOR_SPLIT)


def delta16(x):
    """One fp16 rounding to nearest (mode "f16"): half an ulp, relative 2^-11, absolute floor half the smallest subnormal."""
    x = _d(x).abs()
    return torch.clamp(x * 2.0 ** -11, min=2.0 ** -25)


def _nz(x):
    return (_d(x) != 0).to(F64)


def sum_abs(a, w):
    """S = |a| |w|^T, the natural error scale of a product."""
    return _d(a).abs() @ _d(w).abs().T


def bound_rep(a, w, S=None):
    """Worst case of the three-product form: representation error of either operand against the other's magnitude, plus the
    dropped lo*lo term.  An operand that is exactly zero splits exactly, so it carries no representation error.
    S: sum_abs(a, w) if the caller has it already."""
    a, w = _d(a), _d(w)
    S = sum_abs(a, w) if S is None else S
    return a.abs() @ (delta(w) * _nz(w)).T + (delta(a) * _nz(a)) @ w.abs().T + EPS_SPLIT * S


def bound_acc(a, w, c, S=None):
    """fp32 accumulation: c roundings of relative size 2^-24 against S.  c: scalar, [M, 1] or [1, N]."""
    return EPS_F32 * c * (sum_abs(a, w) if S is None else S)


def c_dense(K):
    return DENSE_C_FACTOR * math.sqrt(3.0 * K)


def c_probe(a):
    """Worst case for a sparse row: three products per non-zero k, each added once."""
    return 3.0 * (_d(a) != 0).sum(dim=1, keepdim=True).to(F64)


def bound_split(a, w, c, S=None):
    S = sum_abs(a, w) if S is None else S
    return bound_rep(a, w, S) + bound_acc(a, w, c, S)


def bound_f32(a, w, S=None):
    """Exact-fp32 paths (fewrow_linear, mode "f32"): accumulation alone, worst case c = K."""
    return bound_acc(a, w, float(a.shape[-1]), S)


def bound_f16(a, w, c, S=None):
    """Single-pass mode "f16": both operands rounded once to fp16, one product."""
    a, w = _d(a), _d(w)
    S = sum_abs(a, w) if S is None else S
    return a.abs() @ (delta16(w) * _nz(w)).T + (delta16(a) * _nz(a)) @ w.abs().T + 2.0 ** -22 * S + bound_acc(a, w, c, S)


def bound_bias(out):
    """One fp32 rounding of an added bias / residual."""
    return EPS_F32 * _d(out).abs()


# ---- first-order composition (the caller multiplies a composed bound by 2 for the second-order remainder) ----
def chain(B1, w2):
    """A second product consumes a first result that is off by B1."""
    return _d(B1) @ _d(w2).abs().T


def layernorm_bound(z, dz, gamma, eps):
    """|dy_i| <= |gamma_i| / sigma * (|dz_i| + mean|dz| + |zhat_i| * mean(|zhat| |dz|)) for y = gamma * zhat + beta."""
    z, dz, gamma = _d(z), _d(dz), _d(gamma)
    mu = z.mean(-1, keepdim=True)
    sig = torch.sqrt(((z - mu) ** 2).mean(-1, keepdim=True) + eps)
    zh = (z - mu) / sig
    return gamma.abs() / sig * (dz + dz.mean(-1, keepdim=True) + zh.abs() * (zh.abs() * dz).mean(-1, keepdim=True))


def layernorm_sigma(z):
    z = _d(z)
    return z.std(dim=-1, unbiased=False)


def ln_eval_bound(z, gamma, beta, eps):
    """fp32 evaluation of a LayerNorm on exact inputs: mean, centring, variance, rsqrt, scale and shift each round once; taken as
    an input perturbation of 2 ulp of (|z| + |mean|) pushed through the first-order LayerNorm bound, plus 4 ulp of the output terms."""
    z, gamma, beta = _d(z), _d(gamma), _d(beta)
    mu = z.mean(-1, keepdim=True)
    y = torch.nn.functional.layer_norm(z, z.shape[-1:], gamma, beta, eps)
    return layernorm_bound(z, 2 * EPS_F32 * (z.abs() + mu.abs()), gamma, eps) + 4 * EPS_F32 * ((y - beta).abs() + y.abs())


def ln_tail(z, Bz, gamma, beta, eps):
    """LayerNorm of a row that is off by Bz, evaluated in fp32."""
    return layernorm_bound(z, Bz, gamma, eps) + ln_eval_bound(z, gamma, beta, eps)


def gelu_eval_bound(z):
    """erf evaluated in fp32 (a few ulp, absolute) times z / 2, and the final product's rounding."""
    z = _d(z)
    return 4 * EPS_F32 * z.abs() + EPS_F32 * torch.nn.functional.gelu(z).abs()


def ffn_ref_and_bound(x, w1, b1, w2, b2, act, ln_in, ln_out, c1, c2, first=bound_split, second=bound_split, h_of=None):
    """out = LN_out?(x + W2 act(W1 LN_in?(x) + b1) + b2) in fp64 and its composed first-order bound (x 2 for the remainder).
    Returns (ref, B, S, hidden pre-activation).  first / second: the bound of each product (bound_split or bound_f16)."""
    Fn = torch.nn.functional
    C = x.shape[1]
    x64, w1, b1, w2, b2 = _d(x), _d(w1), _d(b1), _d(w2), _d(b2)
    if ln_in is not None:
        y = Fn.layer_norm(x64, (C,), _d(ln_in[0]), _d(ln_in[1]), 1e-5)
        By = ln_eval_bound(x64, ln_in[0], ln_in[1], 1e-5)
    else:
        y, By = x64, None
    h = y @ w1.T + b1
    Bh = first(y, w1, c1) + bound_bias(h)
    if By is not None:
        Bh = Bh + chain(By, w1)
    if act == "relu":
        hh, Bhh = torch.relu(h), Bh
    else:
        hh, Bhh = Fn.gelu(h), GELU_LIPSCHITZ * Bh + gelu_eval_bound(h)
    S2 = sum_abs(hh, w2)
    o = x64 + hh @ w2.T + b2
    Bo = chain(Bhh, w2) + second(hh, w2, c2, S2) + 2 * bound_bias(o)
    if ln_out is not None:
        ref = Fn.layer_norm(o, (C,), _d(ln_out[0]), _d(ln_out[1]), 1e-5)
        return ref, 2 * ln_tail(o, Bo, ln_out[0], ln_out[1], 1e-5), S2, h
    return o, 2 * Bo, S2, h


def ffn_probe_operands(which, C, Hd, M, period, ws, as_, seed, launch=0):
    """Operands of the fused-FFN probes (ReLU, b1 = b2 = 0, every operand >= 0 so that ReLU is the identity without a large bias
    that would put 2^-20 |b1| into the bound).
    first: K-block rows x, dense W1 >= 0, W2 a 0 / 1 selection (output i <- hidden i + C * launch).  second: W1 a 0 / 1 selection
    (hidden j + C * launch <- x[j], the other hidden units idle), so the hidden rows are K-block rows of the second walk; W2 dense.
    Hd / C launches see every hidden unit, 8 per row, undiluted."""
    g = torch.Generator().manual_seed(int(seed))
    x = kblock_probe(M, C, as_, period, seed=seed).abs()
    i = torch.arange(min(C, Hd))
    sel = i + C * launch if Hd >= C else i
    if which == "first":
        w1 = torch.randn(Hd, C, generator=g).abs() / math.sqrt(C) * ws
        w2 = torch.zeros(C, Hd)
        w2[i, sel] = 1.0
    else:
        w1 = torch.zeros(Hd, C)
        w1[sel, i] = 1.0
        w2 = torch.randn(C, Hd, generator=g) / math.sqrt(Hd) * ws
    c1 = c_probe(x)
    if which == "first":
        c2 = 3.0 * (w2 != 0).sum(1).double()[None, :]
    else:
        c2 = 3.0 * ((x.double() @ w1.double().T) != 0).sum(1, keepdim=True).double()
    return x, w1, torch.zeros(Hd), w2, torch.zeros(C), c1, c2


def softmax_v_bound(p, v, b_score, c, product=None):
    """softmax(s) @ v with scores off by at most b_score [rows, 1]: 2 max_j(B_score) sum_j p_j |v_j| + bound(p, v).
    p [rows, L], v [L, D] (so the second product is p @ v = p @ (v.T).T).  product: the second product's bound (bound_split)."""
    p, v = _d(p), _d(v)
    return 2.0 * b_score * (p @ v.abs()) + (product or bound_split)(p, v.T, c)


# ---- operands ----
def dense_operands(M, N, K, wscale, ascale, seed):
    """randn activations, randn / sqrt(K) weights, as fp32."""
    g = torch.Generator().manual_seed(int(seed))
    a = torch.randn(M, K, generator=g) * ascale
    w = torch.randn(N, K, generator=g) / math.sqrt(K) * wscale
    return a, w


def decades_operands(M, N, K, seed):
    """Four decades of dynamic range along K."""
    g = torch.Generator().manual_seed(int(seed))
    a = torch.randn(M, K, generator=g) * torch.logspace(-2, 2, K)[None, :]
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    return a, w


def probe_blocks(M, K, period, shift=0):
    """k-block of row r: (r % period + step * (r // period) + shift) % (K / 8).  With at least K / 8 row tiles step is 1 and every
    (row-in-tile, k-block) pair occurs; with fewer (row count capped) step grows so that every k-block still occurs in some row.
    (r + r // period, without the r % period, would visit only gcd-many blocks per row-in-tile whenever period + 1 and K / 8 share a
    factor, e.g. period 128 at K = 96.)"""
    nb = K // 8
    r = torch.arange(M)
    tiles = (M + period - 1) // period
    step = max(1, -(-nb // tiles))
    return (r % period + step * (r // period) + shift) % nb


def kblock_probe(M, K, scale, period, seed=0, shift=0):
    """Rows whose non-zeros are the 8 consecutive k of block probe_blocks(r): a defect confined to one k index or one 8-half
    fragment is the whole of some row's product instead of 1/K of it."""
    assert K % 8 == 0
    g = torch.Generator().manual_seed(int(seed))
    a = torch.zeros(M, K)
    r = torch.arange(M)
    blk = probe_blocks(M, K, period, shift)
    for j in range(8):
        a[r, blk * 8 + j] = torch.randn(M, generator=g) * scale
    return a


def im2col(x, T, H, W, Cin, k, s, p):
    """x [T*H*W, Cin] channels-last -> [T*Ho*Wo, k*k*Cin] with column (ky*k + kx)*Cin + c (the packed weight's K order)."""
    xx = torch.nn.functional.pad(x.view(T, H, W, Cin), (0, 0, p, p, p, p))
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    taps = [xx[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s] for ky in range(k) for kx in range(k)]
    return torch.stack(taps, 3).reshape(T * Ho * Wo, k * k * Cin)


def conv_cases(T, H, W, Cin, N, k, seed, probe_frames=None):
    """(kind, weight scale, activation scale, frames, x [frames*H*W, Cin], w [N, k*k*Cin]) of a convolution family: the dense sweep,
    the four-decade case (scales None: the range runs along the channels of every tap), and the probe -- frame t holds the 8
    channels of block t % (Cin / 8) only, max(T, Cin / 8) frames so that every block occurs, and for k > 1 only at the pixels of
    a lattice of pitch 3 (shifted from frame to frame): a k <= 3 window then holds at most one non-zero pixel, so an output row has
    8 non-zeros, those of ONE tap, and the outputs around a lattice pixel walk through all k*k taps.  (With every pixel non-zero
    a row would sum k*k*8 terms and one wrong lo would be 1/9 as visible.)"""
    K = k * k * Cin
    for j, (ws, as_) in enumerate(DENSE_SCALES):
        g = torch.Generator().manual_seed(seed * 16 + j)
        x = torch.randn(T * H * W, Cin, generator=g) * as_
        w = torch.randn(N, K, generator=g) / math.sqrt(K) * ws
        yield "dense", ws, as_, T, x, w
    g = torch.Generator().manual_seed(seed * 16 + 7)
    x = torch.randn(T * H * W, Cin, generator=g) * torch.logspace(-2, 2, Cin)[None, :]
    yield "dense", None, None, T, x, torch.randn(N, K, generator=g) / math.sqrt(K)
    Tp = probe_frames or max(T, Cin // 8)
    for j, (ws, as_) in enumerate(PROBE_SCALES):
        g = torch.Generator().manual_seed(seed * 16 + 8 + j)
        x = torch.zeros(Tp, H, W, Cin)
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        for t in range(Tp):
            b = t % (Cin // 8)
            on = ((yy + t) % 3 == 0) & ((xx + t // 3) % 3 == 0) if k > 1 else torch.ones(H, W, dtype=torch.bool)
            x[t, :, :, 8 * b:8 * b + 8] = torch.randn(H, W, 8, generator=g) * as_ * on[:, :, None]
        w = torch.randn(N, K, generator=g) / math.sqrt(K) * ws
        yield "probe", ws, as_, Tp, x.view(-1, Cin), w


def probe_rows(K, period, cap=8192):
    """Enough rows that every (row-in-tile, k-block) pair occurs, capped."""
    return min(period * (K // 8), cap)


# ---- emulation ----
def rtz16(x):
    """fp32 -> fp16 truncated toward zero, returned as fp32."""
    h = x.half()
    over = h.float().abs() > x.abs()
    b = h.view(torch.int16)
    b = torch.where(over, b - 1, b)
    return b.view(torch.half).float()


def split(x, rtz=True):
    hi = rtz16(x) if rtz else x.half().float()
    r = x - hi
    lo = rtz16(r) if rtz else r.half().float()
    return hi, lo


LOCAL_MUTANTS = ("lo_zero_k16", "lo_zero_one_k", "wlo_misplaced_frag", "wlo_tail")
GLOBAL_MUTANTS = ("drop_alo_whi", "drop_ahi_wlo", "flush_subnormal_lo", "single_pass")


def emulate_split(a, w, rtz=True, mutant=None):
    """The documented arithmetic on the CPU (fp32 operands, fp16 halves, three products, fp32 accumulation), optionally with
    one defect of the kind a wrong index in a pack kernel or a fragment load produces."""
    a, w = a.float(), w.float()
    K = a.shape[1]
    ah, al = split(a, rtz)
    wh, wl = split(w, rtz)
    mm = lambda x, y: x @ y.T
    if mutant == "single_pass":
        return mm(a.half().float(), w.half().float())
    if mutant == "flush_subnormal_lo":
        al = torch.where(al.abs() < 2.0 ** -14, torch.zeros_like(al), al)
        wl = torch.where(wl.abs() < 2.0 ** -14, torch.zeros_like(wl), wl)
    elif mutant == "lo_zero_k16":
        al = al.clone()
        al[:, 16:32] = 0
    elif mutant == "lo_zero_one_k":
        al = al.clone()
        al[:, 5] = 0
    elif mutant == "wlo_misplaced_frag":
        wl = wl.clone()
        wl[7, 40:48] = wl[7, 32:40]
    elif mutant == "wlo_tail":
        wl = wl.clone()
        wl[:, K - 8:] = 0
    elif mutant not in (None, "drop_alo_whi", "drop_ahi_wlo"):
        raise ValueError(mutant)
    out = mm(ah, wh)
    if mutant != "drop_ahi_wlo":
        out = out + mm(ah, wl)
    if mutant != "drop_alo_whi":
        out = out + mm(al, wh)
    return out


def worst(out, ref, B):
    """(max err / B, flat index of the worst element); NaN counts as infinitely wrong."""
    ratio = ((_d(out) - _d(ref)).abs() / _d(B)).nan_to_num(nan=float("inf"))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i
