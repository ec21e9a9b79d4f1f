#!/usr/bin/env python3
"""Per-layer timing of the implicit-GEMM conv kernels at the 64x64 (c2) shapes: forward,
data-gradient, weight-gradient, with achieved TFLOP/s against the 157.3 TF fp32-MFMA peak.
`bench_layers.py up2fold`: A/B of the upsampled convs' data gradient, conv + upsample adjoint against the fused call."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
from hipvae import functional as HF  # noqa: E402

LAYERS = [  # Ci, Co, S, KS
    (3, 64, 64, 5), (64, 128, 32, 3), (128, 128, 32, 3), (128, 256, 16, 3), (256, 256, 16, 3),
    (256, 512, 8, 3), (512, 512, 8, 3), (512, 512, 4, 3), (64, 64, 64, 3), (128, 64, 32, 3), (64, 3, 64, 5),
]


def timeit(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    d = torch.device("cuda:0")
    print(f"{'layer':>22} {'GF':>7} | {'fwd ms':>8} {'TF':>6} | {'dgrad ms':>8} {'TF':>6} | {'wgrad ms':>8} {'TF':>6}")
    tot = [0.0, 0.0, 0.0, 0.0]
    for Ci, Co, S, KS in LAYERS:
        x = torch.randn(B, Ci, S, S, device=d)
        w = torch.randn(Co, Ci, KS, KS, device=d) * 0.05
        dy = torch.randn(B, Co, S, S, device=d)
        wp, wpt = HF.pack_weight(w, 0), HF.pack_weight(w, 1)
        gf = 2.0 * B * S * S * Co * Ci * KS * KS * 1e-9
        tf = timeit(lambda: HF.conv_fwd_raw(x, wp, None, B, Ci, S, S, Co, KS, False))
        td = timeit(lambda: HF.conv_fwd_raw(dy, wpt, None, B, Co, S, S, Ci, KS, False))
        tw = timeit(lambda: HF.conv_wgrad_raw(x, dy, B, Ci, S, S, Co, KS, False))
        extra = ""
        if HF.lib.itcv_conv2d_bf16s_supported(Ci, Co, KS) and HF.lib.itcv_conv2d_bf16s_supported(Co, Ci, KS):
            ref = HF.conv_fwd_raw(x, wp, None, B, Ci, S, S, Co, KS, False)
            for mode in ("bf16x3", "bf16x6"):
                HF.set_conv_math(mode)
                t3 = timeit(lambda: HF.conv_apply(x, w, w, 0, None, B, Ci, S, S, Co, KS, False))
                err = float((HF.conv_apply(x, w, w, 0, None, B, Ci, S, S, Co, KS, False) - ref).abs().max() / ref.abs().max())
                extra += f" | {mode} {t3*1e3:6.3f} ms {gf/t3*1e-3:6.1f} TFeq err {err:.1e}"
                if HF.lib.itcv_conv2d_wgrad_bf16s_supported(Ci, S, S, Co, KS):
                    refw = None
                    HF.set_conv_math("fp32"); refw = HF.conv_wgrad_raw(x, dy, B, Ci, S, S, Co, KS, False); HF.set_conv_math(mode)
                    tw3 = timeit(lambda: HF.conv_wgrad_raw(x, dy, B, Ci, S, S, Co, KS, False))
                    errw = float((HF.conv_wgrad_raw(x, dy, B, Ci, S, S, Co, KS, False) - refw).abs().max() / refw.abs().max())
                    extra += f" wg {tw3*1e3:6.3f} ms {gf/tw3*1e-3:6.1f} err {errw:.1e}"
            HF.set_conv_math("fp32")
        print(f"{Ci:4d}->{Co:4d}@{S:3d} k{KS} B{B:3d} {gf:7.2f} | {tf*1e3:8.3f} {gf/tf*1e-3:6.1f} | "
              f"{td*1e3:8.3f} {gf/td*1e-3:6.1f} | {tw*1e3:8.3f} {gf/tw*1e-3:6.1f}" + extra)
        tot[0] += gf; tot[1] += tf; tot[2] += td; tot[3] += tw
    print(f"{'sum':>22} {tot[0]:7.2f} | {tot[1]*1e3:8.3f} {tot[0]/tot[1]*1e-3:6.1f} | {tot[2]*1e3:8.3f} "
          f"{tot[0]/tot[2]*1e-3:6.1f} | {tot[3]*1e3:8.3f} {tot[0]/tot[3]*1e-3:6.1f}")


def up2_fold_ab():
    """`bench_layers.py up2fold`: data gradient of the c2 decoder's upsampled convs (f16x3 planes) at 64 and 128 images,
    the two calls (band conv into the H x W tensor + itcv_upsample2_bwd) against the fused entry point.  Per form 4 calls
    are captured into a graph; median (and min) of 50 replays, us per call."""
    from hipvae.abi import call, ptr, stream
    d, fmt, calls, reps = torch.device("cuda:0"), HF.F16X2, 4, 50

    def timed(once):
        for _ in range(3):
            once()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(calls):
                once()
        for _ in range(3):
            graph.replay()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / calls)
        ts.sort()
        return ts[len(ts) // 2], ts[0]

    print(f"{'dy -> dx @ size':>20} {'B':>4} {'hi MB':>7} | {'conv+adjoint us':>16} {'min':>7} | {'fused us':>9} {'min':>7} | saved")
    for D, X, S in ((64, 64, 64), (64, 128, 32), (128, 256, 16)):
        for B in (64, 128):
            dy = torch.randn(B, D, S, S, device=d) * 1e-3
            w = torch.randn(D, X, 3, 3, device=d) * 0.05
            dyp, wp = HF.split_planes(dy, fmt, gradient=True), HF.pack_weight_bf16s(w, 1, fmt)
            hi, lo = torch.empty(B, X, S, S, device=d), torch.empty(B, X, S // 2, S // 2, device=d)
            lo2 = torch.empty_like(lo)
            assert HF.lib.itcv_conv2d_dgrad_up2_supported(B, D, S, S, X, 3, fmt, B)

            def two():
                call("itcv_conv2d_fwd_bf16p_st", ptr(dyp), ptr(wp), None, ptr(hi), B, D, S, S, X, 3, 0, fmt, None, None, 0, stream())
                call("itcv_upsample2_bwd", ptr(hi), ptr(lo), B * X, S // 2, S // 2, stream())

            def one():
                call("itcv_conv2d_dgrad_up2_bf16p", ptr(dyp), ptr(wp), ptr(lo2), B, D, S, S, X, 3, fmt, 0, B, None, 0, stream())

            (t2, m2), (t1, m1) = timed(two), timed(one)
            assert torch.equal(lo, lo2)
            print(f"{D:4d} ->{X:4d} @ {S:3d}x{S:<3d} {B:4d} {hi.numel() * 4 / 1e6:7.1f} | {t2:16.1f} {m2:7.1f} | {t1:9.1f} {m1:7.1f} | "
                  f"{t2 - t1:6.1f} us", flush=True)


if __name__ == "__main__":
    up2_fold_ab() if sys.argv[1:2] == ["up2fold"] else main()
