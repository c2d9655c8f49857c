"""Split 3x3 convolution (tce_conv3x3_split_f32) against the un-split launch (tce_conv3x3_f32) at the pixel decoder's map sizes:
time of the plan's own piece count and of forced ones (tce_debug_conv3x3_set_pieces), max |difference| to the un-split output."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tce_rvos_amd  # noqa: F401
from tce_rvos_amd import ops
from tce_rvos_amd._lib import lib


def timeit(fn, n=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    l = lib()
    g = torch.Generator(device="cpu").manual_seed(0)
    w_cl = (torch.randn(256, 2304, generator=g) / 48.0).cuda()
    b = torch.randn(256, generator=g).cuda()
    pk = ops.conv3x3_pack(w_cl, 256)
    ws = torch.empty(12 * 256 * 128 * 256, device="cuda")  # any forced plan up to 12 pieces of a sub-round launch
    stream = torch.cuda.current_stream().cuda_stream
    for (T, H, W) in ((5, 90, 160), (5, 45, 80), (8, 96, 160), (10, 120, 107), (8, 45, 80)):
        M = T * H * W
        x = torch.randn(M, 256, generator=g).cuda()
        o1, o2 = torch.empty(M, 256, device="cuda"), torch.empty(M, 256, device="cuda")

        def unsplit():
            l.tce_conv3x3_f32(x.data_ptr(), 256, pk.data_ptr(), b.data_ptr(), o1.data_ptr(), 256, T, H, W, 256, 256, stream)

        def split():
            rc = l.tce_conv3x3_split_f32(x.data_ptr(), 256, pk.data_ptr(), b.data_ptr(), o2.data_ptr(), 256, T, H, W, 256, 256,
                                         ws.data_ptr(), ws.numel(), stream)
            assert rc == 0, l.tce_last_error()
        t0 = timeit(unsplit)
        auto = l.tce_conv3x3_split_pieces(M, 256, 256)
        res = []
        for p in (0, 2, 3, 4, 5, 6):
            l.tce_debug_conv3x3_set_pieces(p)
            t = timeit(split)
            res.append(f"{'plan' if p == 0 else p}:{t:6.1f}")
        l.tce_debug_conv3x3_set_pieces(0)
        t0 = min(t0, timeit(unsplit))  # again after the split runs: the first timing of a shape can run at a lower clock
        split()
        unsplit()
        torch.cuda.synchronize()
        d = (o1 - o2).abs().max().item() / o1.abs().max().item()
        print(f"T={T} {H}x{W} ({M} px): un-split {t0:6.1f} us   split (plan = {auto} pieces) us by pieces: {'  '.join(res)}   "
              f"max|d|/max|out| {d:.2e}", flush=True)


if __name__ == "__main__":
    main()
