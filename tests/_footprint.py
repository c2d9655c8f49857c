"""Slab harness: holds an access model (hazard.MODELS) to what the kernel it describes really touches.

A *slab* is ONE uint8 tensor that holds every buffer of a case -- inputs, weights, packed streams, outputs, workspaces,
counters -- with a guard band before and after each, so whatever a launch touches beyond its buffers is still memory the
test owns and looks at.  Three properties are checked against the byte intervals the model itself reports for the real
call (recorded, not restated):

  W  writes stay inside the model: with the slab filled with a canary word, every byte outside the union of modelled
     writes is bit-unchanged after the run (guards, pad columns, batch gaps, every input, every weight).  Two canaries.
  O  outputs are fully written: no canary word remains inside a modelled write range, except in buffers the case
     declares as workspace / counters.
  R  results do not depend on unmodelled bytes: with everything outside the union of modelled reads filled with zero
     bytes / a quiet NaN / a large negative finite pattern, the modelled output bytes are bit-identical.

Pure torch + numpy: the same code runs on CPU slabs with plain functions standing in for kernels (test_footprint_cpu.py);
only `recorder`, which the GPU cases of the stage models share, needs a device.
"""
import numpy as np
import torch

from tce_rvos_amd import hazard

ALIGN = 256            # what ops.Arena gives
GUARD_MIN = 256 << 10  # bytes; and at least GUARD_ROWS rows of the buffer's pitch
GUARD_ROWS = 128
CANARIES = (0xC3A5965B, 0x5A6B3CC7)  # neither a plausible float result, nor 0/1 bytes, nor a small integer
# R fills: the bit pattern of every 4-byte word outside the modelled reads
FILLS = (("zero", 0x00000000),
         ("qnan", 0x7FC00000),
         ("big", 0xFE967699))  # -1.0e38: sign and exponent set, so a stray term neither cancels nor hides in max / min


class FootprintError(AssertionError):
    pass


def _i32(word):
    return int(np.array([word], dtype=np.uint32).view(np.int32)[0])


class Buf:
    __slots__ = ("name", "off", "nbytes", "pitch_bytes", "tensor")

    def __repr__(self):
        return f"{self.name}@{self.off:#x}+{self.nbytes}"


class Slab:
    """Bump allocator over one uint8 tensor.  `begin(word)` starts a case: every byte handed out from then on (guards
    included) is first filled with `word`."""

    def __init__(self, nbytes, device="cpu", guard_min=GUARD_MIN):
        """guard_min below GUARD_MIN is for stand-ins on the CPU only (their overruns are a few bytes); GPU cases keep the default."""
        self.guard_min = int(guard_min)
        nbytes = (int(nbytes) + 3) // 4 * 4
        raw = torch.zeros(nbytes + ALIGN, dtype=torch.uint8, device=device)  # one allocation; the slab starts on a 256-byte line
        shift = -raw.data_ptr() % ALIGN
        self.mem = raw[shift:shift + nbytes]
        self.words = self.mem.view(torch.int32)
        self.device = self.mem.device
        self.base = self.mem.data_ptr()
        if self.base % ALIGN:
            raise FootprintError("slab base is not 256-byte aligned")
        self.begin(0)

    def begin(self, word):
        self.word = int(word)
        self.off = 0      # end of the last buffer
        self.used = 0     # end of the last guard (filled up to here)
        self.tail = 0     # guard the last buffer asks for
        self.bufs = []
        self._seed = 0

    def guard_for(self, pitch_bytes):
        g = max(self.guard_min, GUARD_ROWS * int(pitch_bytes))
        return (g + ALIGN - 1) // ALIGN * ALIGN

    def alloc(self, name, shape, dtype=torch.float32, pitch=None, bstride=None, align=ALIGN):
        """shape (n,), (rows, cols) or (batch, rows, cols); pitch = row pitch in elements (> cols leaves pad columns),
        bstride = batch stride in elements (> rows * pitch leaves inter-batch gaps).  Returns the strided view."""
        shape = tuple(int(s) for s in shape)
        es = torch.empty((), dtype=dtype).element_size()
        cols = shape[-1]
        rows = shape[-2] if len(shape) >= 2 else 1
        batch = shape[0] if len(shape) == 3 else 1
        if len(shape) > 3:
            raise ValueError("slab buffers are 1-D, 2-D or 3-D")
        pitch = cols if pitch is None else int(pitch)
        bstride = rows * pitch if bstride is None else int(bstride)
        if pitch < cols or (batch > 1 and bstride < rows * pitch):
            raise ValueError("pitch / batch stride smaller than the extent")
        span = ((batch - 1) * bstride + (rows - 1) * pitch + cols) * es
        guard = self.guard_for(pitch * es if len(shape) >= 2 else es)  # a 1-D buffer has no rows: the 256 KiB minimum
        start = self.off + max(guard, self.tail)
        start = (start + align - 1) // align * align
        end = start + span
        used = (end + guard + 3) // 4 * 4
        if used > self.mem.numel():
            raise FootprintError(f"slab too small: {name} needs {used} bytes, slab has {self.mem.numel()}")
        self.words[self.used // 4:used // 4].fill_(_i32(self.word))
        b = Buf()
        b.name, b.off, b.nbytes, b.pitch_bytes = name, start, span, pitch * es
        flat = self.mem[start:end].view(dtype)
        strides = {1: (1,), 2: (pitch, 1), 3: (bstride, pitch, 1)}[len(shape)]
        b.tensor = torch.as_strided(flat, shape, strides)
        self.bufs.append(b)
        self.off, self.used, self.tail = end, used, guard
        return b.tensor

    # deterministic contents: the same sequence of requests gives the same values in every run of a case
    def _gen(self):
        self._seed += 1
        return torch.Generator(device="cpu").manual_seed(1000 + self._seed)

    def randn(self, name, shape, scale=1.0, shift=0.0, **kw):
        t = self.alloc(name, shape, **kw)
        t.copy_((torch.randn(tuple(t.shape), generator=self._gen()) * scale + shift).to(self.device))
        return t

    def rand(self, name, shape, lo=0.0, hi=1.0, **kw):
        t = self.alloc(name, shape, **kw)
        t.copy_((torch.rand(tuple(t.shape), generator=self._gen()) * (hi - lo) + lo).to(self.device))
        return t

    def put(self, name, values, dtype=None, **kw):
        v = torch.as_tensor(values)
        if dtype is not None:
            v = v.to(dtype)
        t = self.alloc(name, tuple(v.shape), dtype=v.dtype, **kw)
        t.copy_(v.to(self.device))
        return t

    def randint(self, name, shape, lo, hi, dtype=torch.int64, **kw):
        t = self.alloc(name, shape, dtype=dtype, **kw)
        t.copy_(torch.randint(lo, hi, tuple(t.shape), generator=self._gen()).to(dtype).to(self.device))
        return t

    def buf(self, name):
        for b in self.bufs:
            if b.name == name:
                return b
        raise KeyError(name)

    # ------------------------------------------------------------------------------------------------------------
    # interval helpers (offsets into the slab), built on hazard.strided / union / merge
    # ------------------------------------------------------------------------------------------------------------
    def to_offsets(self, sets, what="access"):
        """Union of absolute interval sets -> merged slab offsets.  A range outside the case's bytes is an error: the case
        forgot a buffer (or the model describes memory the call was never given)."""
        iv = hazard.union(*[np.asarray(s, dtype=np.int64).reshape(-1, 2) for s in sets]) - self.base
        if len(iv) and (iv[0, 0] < 0 or iv[-1, 1] > self.used):
            bad = iv[(iv[:, 0] < 0) | (iv[:, 1] > self.used)][0]
            raise FootprintError(f"modelled {what} [{int(bad[0]):#x}, {int(bad[1]):#x}) lies outside the slab's "
                                 f"{self.used:#x} bytes in use: the case forgot a buffer")
        return iv

    def complement(self, iv):
        """[0, used) minus a merged interval set."""
        iv = hazard.merge(np.asarray(iv, dtype=np.int64).reshape(-1, 2))
        if not len(iv):
            return np.array([[0, self.used]], dtype=np.int64)
        lo = np.concatenate([[0], iv[:, 1]])
        hi = np.concatenate([iv[:, 0], [self.used]])
        keep = hi > lo
        return np.stack([lo[keep], hi[keep]], 1)

    def mask(self, iv):
        """bool [used]: bytes inside the merged (disjoint) interval set."""
        n = self.used
        d = torch.zeros(n + 1, dtype=torch.int8, device=self.device)
        if len(iv):
            iv = hazard.merge(np.asarray(iv, dtype=np.int64).reshape(-1, 2))
            d[torch.from_numpy(np.ascontiguousarray(iv[:, 0])).to(self.device)] = 1
            e = torch.from_numpy(np.ascontiguousarray(iv[:, 1])).to(self.device)
            d[e] -= 1  # ends are distinct from starts after merging (touching intervals are merged)
        return torch.cumsum(d[:n], 0, dtype=torch.int8) > 0

    def pattern(self, word):
        """uint8 [used]: `word` repeated on the slab's 4-byte grid."""
        return torch.full((self.used // 4,), _i32(word), dtype=torch.int32, device=self.device).view(torch.uint8)

    def fill(self, iv, word):
        m = self.mask(iv)
        cur = self.mem[:self.used]
        cur.copy_(torch.where(m, self.pattern(word), cur))

    def where(self, off):
        """'buffer +offset' / 'guard before buffer' for a slab offset."""
        prev = None
        for b in self.bufs:
            if off < b.off:
                return (f"guard {b.off - off} bytes before {b.name}" if prev is None or off - (prev.off + prev.nbytes) >= b.off - off
                        else f"guard {off - (prev.off + prev.nbytes)} bytes after the end of {prev.name}") + f" (slab offset {off:#x})"
            if off < b.off + b.nbytes:
                rel = off - b.off
                return f"{b.name} + {rel} bytes (row {rel // b.pitch_bytes}, byte {rel % b.pitch_bytes} of its pitch; slab offset {off:#x})"
            prev = b
        return f"guard {off - (prev.off + prev.nbytes)} bytes after the end of {prev.name} (slab offset {off:#x})"

    def extent_iv(self, names):
        """Full extents (pads and gaps included) of the named buffers."""
        iv = [[b.off, b.off + b.nbytes] for b in self.bufs if b.name in names]
        return hazard.merge(np.array(iv, dtype=np.int64).reshape(-1, 2))


def _minus(a, b):
    """merged interval set a minus merged interval set b"""
    if not len(a) or not len(b):
        return a
    pts = np.concatenate([np.stack([a[:, 0], np.ones(len(a), np.int64)], 1), np.stack([a[:, 1], -np.ones(len(a), np.int64)], 1),
                          np.stack([b[:, 0], -2 * np.ones(len(b), np.int64)], 1), np.stack([b[:, 1], 2 * np.ones(len(b), np.int64)], 1)])
    pts = pts[np.lexsort((pts[:, 1], pts[:, 0]))]
    out, depth, start = [], 0, None
    for x, d in pts:
        was = depth == 1
        depth += d
        if not was and depth == 1:
            start = x
        elif was and depth != 1 and x > start:
            out.append((start, x))
    return hazard.merge(np.array(out, dtype=np.int64).reshape(-1, 2))


def _intersect(a, b):
    return _minus(a, _minus(a, b))


def _first(mask):
    return int(torch.nonzero(mask)[0, 0])


def check_case(slab, build, record, exempt=(), atomic=None, scratch=(), props="WOR", sync=None, label="case"):
    """Runs one case.

    build(slab) -> fn   allocates every buffer in the slab, places the inputs (and runs whatever prepares them, e.g. a
                        weight pack), and returns the call under test;
    record(fn, dry) -> (reads, writes)   runs fn (dry: without launching) and returns the MODEL's absolute byte intervals
                        for it, as lists of interval sets (hazard.recording on the GPU);
    exempt              names of buffers exempt from O (workspaces, counters);
    atomic              None, or (names, rtol, atol_scale): the named output buffers are accumulated with float atomics, so for THEM R
                        asks for finite values that agree with the zero fill within rtol * |ref| + atol_scale * max|ref of that
                        buffer| instead of equal bits; every other output of the case keeps equal bits;
    scratch             names of buffers whose previous content is no input even where the model lists them as read AND written
                        (workspaces): R fills them too, so a launch that consumes workspace bytes it did not produce is seen.
    Returns a dict of what was checked; raises FootprintError naming property, buffer and byte offset."""
    sync = sync or (lambda: None)
    info = {"W": 0, "O": 0, "R": 0, "exempt": sorted(exempt)}

    # ---- W and O: canary everywhere, twice ----
    for canary in (CANARIES if ("W" in props or "O" in props) else ()):
        slab.begin(canary)
        fn = build(slab)
        sync()
        before = slab.mem[:slab.used].clone()
        rd, wr = record(fn, False)
        sync()
        rd, wr = slab.to_offsets(rd, "read"), slab.to_offsets(wr, "write")
        wmask = slab.mask(wr)
        after = slab.mem[:slab.used]
        if "W" in props:
            bad = (after != before) & ~wmask
            if bool(bad.any()):
                off = _first(bad)
                raise FootprintError(f"{label}: W violated (canary {canary:#010x}): byte changed outside the modelled writes at "
                                     f"{slab.where(off)}; {int(bad.sum())} such bytes")
            info["W"] += 1
        if "O" in props:
            wm = wmask.clone()
            ex = slab.extent_iv(set(exempt))
            if len(ex):
                wm &= ~slab.mask(ex)
            full = wm.view(-1, 4).all(1)  # words wholly inside a modelled output
            hole = full & (slab.words[:slab.used // 4] == _i32(canary))
            if bool(hole.any()):
                off = _first(hole) * 4
                raise FootprintError(f"{label}: O violated (canary {canary:#010x}): modelled output never written at "
                                     f"{slab.where(off)}; {int(hole.sum())} such words")
            info["O"] += 1
        info["read_bytes"] = int((rd[:, 1] - rd[:, 0]).sum()) if len(rd) else 0
        info["written_bytes"] = int((wr[:, 1] - wr[:, 0]).sum()) if len(wr) else 0
        body = sum(b.nbytes for b in slab.bufs)
        ext = slab.extent_iv({b.name for b in slab.bufs})
        inside = int((slab.mask(ext) & ~slab.mask(hazard.union(rd, wr))).sum())
        info["guard_bytes"] = slab.used - body
        info["pad_bytes"] = inside  # bytes inside buffers that neither model touches: pad columns, batch gaps, omitted operands
        info["slab_bytes"] = slab.used

    # ---- R: everything outside the modelled reads is zero / NaN / large ----
    if "R" in props:
        outs = []
        for fname, word in FILLS:
            slab.begin(0)
            fn = build(slab)
            sync()
            rd, wr = record(fn, True)
            rd, wr = slab.to_offsets(rd, "read"), slab.to_offsets(wr, "write")
            slab.fill(hazard.union(slab.complement(rd), slab.extent_iv(set(scratch))), word)
            sync()
            rd2, wr2 = record(fn, False)
            sync()
            if not (np.array_equal(slab.to_offsets(rd2), rd) and np.array_equal(slab.to_offsets(wr2), wr)):
                raise FootprintError(f"{label}: the model reported different intervals for the dry and the real run")
            # compared: every modelled write, except workspace bytes the model also lists as read -- those now hold the fill
            # wherever the launch leaves them unwritten (O exempts exactly that), so they are inputs under test here, not results
            wr = _minus(wr, _intersect(slab.extent_iv(set(scratch)), rd))
            outs.append((fname, slab.mem[:slab.used][slab.mask(wr)].clone(), wr))
        ref, wr = outs[0][1], outs[0][2]
        amask = None
        if atomic is not None:
            names, rtol, ascale = atomic
            amask = slab.mask(slab.extent_iv(set(names)))[slab.mask(wr)]  # over the written bytes, in slab order
        for fname, o, _ in outs[1:]:
            diff = o != ref
            if amask is not None:
                diff &= ~amask
            if bool(diff.any()):
                k = _first(diff)
                lens = wr[:, 1] - wr[:, 0]  # k-th written byte -> slab offset
                cum = np.cumsum(lens)
                j = int(np.searchsorted(cum, k, side="right"))
                off = int(wr[j, 0] + (k - (cum[j - 1] if j else 0)))
                raise FootprintError(f"{label}: R violated: output differs between the 'zero' and the '{fname}' fill of the bytes "
                                     f"outside the modelled reads, first at {slab.where(off)}; {int(diff.sum())} bytes differ")
            if amask is not None:
                for bname in names:
                    bb = slab.buf(bname)
                    sel = slab.mask(np.array([[bb.off, bb.off + bb.nbytes]])) & slab.mask(wr)
                    selw = sel[slab.mask(wr)]
                    a, b_ = o[selw].view(torch.float32).double(), ref[selw].view(torch.float32).double()
                    if not bool(torch.isfinite(a).all()):
                        raise FootprintError(f"{label}: R violated: non-finite values in {bname} under the '{fname}' fill")
                    tol = rtol * b_.abs() + ascale * float(b_.abs().max())
                    if bool(((a - b_).abs() > tol).any()):
                        raise FootprintError(f"{label}: R violated: {bname} under the '{fname}' fill leaves the atomics tolerance "
                                             f"(max diff {float((a - b_).abs().max()):.3e})")
        info["R"] = len(outs)
    return info


def recorder(*names):
    """-> record(fn, dry) for check_case on the GPU: what fn launches goes through hazard.recording(), so the intervals are the
    model's own for the real call (not restated), and fn must launch exactly the entry points `names`, in this order."""
    def record(fn, dry):
        with hazard.recording(dry=dry) as rec:
            fn()
        torch.cuda.synchronize()
        assert [x.name for x in rec.launches] == list(names)
        return [x.reads for x in rec.launches], [x.writes for x in rec.launches]
    return record


def first_touched_outside(buf, writes, word, window=64 << 20):
    """buf: a uint8 device tensor that was filled with `word` (on its own 4-byte grid); writes: merged ABSOLUTE intervals.
    Walks the complement of the writes inside buf, one window at a time on the device (no mask of the whole buffer), and
    returns (offset, count) of the bytes that no longer hold the fill, or None."""
    base, n = buf.data_ptr(), buf.numel()
    iv = hazard.merge(np.asarray(writes, dtype=np.int64).reshape(-1, 2)) - base
    iv = iv[(iv[:, 1] > 0) & (iv[:, 0] < n)] if len(iv) else iv
    iv = np.clip(iv, 0, n)
    pat = torch.full((window // 4,), _i32(word), dtype=torch.int32, device=buf.device).view(torch.uint8)
    first, count = None, 0
    for w0 in range(0, n, window):
        w1 = min(n, w0 + window)
        lo, hi = np.searchsorted(iv[:, 1], w0, side="right"), np.searchsorted(iv[:, 0], w1, side="left")
        loc = np.clip(iv[lo:hi], w0, w1) - w0
        if len(loc) == 1 and loc[0, 0] == 0 and loc[0, 1] == w1 - w0:
            continue  # the window is written in full
        bad = buf[w0:w1] != pat[:w1 - w0]
        if len(loc):
            d = torch.zeros(w1 - w0 + 1, dtype=torch.int8, device=buf.device)
            d[torch.from_numpy(np.ascontiguousarray(loc[:, 0])).to(buf.device)] = 1
            d[torch.from_numpy(np.ascontiguousarray(loc[:, 1])).to(buf.device)] -= 1
            bad &= ~(torch.cumsum(d[:w1 - w0], 0, dtype=torch.int8) > 0)
        k = int(bad.sum())
        if k:
            if first is None:
                first = w0 + _first(bad)
            count += k
    return None if first is None else (first, count)
