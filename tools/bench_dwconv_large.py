"""Per-shape timing of the large depthwise Conv3d kernels (csrc/depthwise_large.hip) at the production shapes of
FocalNetUNETR-48 at 96^3, batch 2, bf16 -- (C, grid) = (48, 48^3), (96, 24^3), (192, 12^3), (384, 6^3), K = 9 and 11 --:
forward, input gradient, weight gradient, each next to torch.nn.functional.conv3d(groups=C) (bf16, channels_last_3d: the
path the reference takes) in the same process, the two alternating sample by sample.  Device events, warm-up, a timed
window of at least one second per figure.  Columns: us per call, and for the forward the share of the fp32 vector bound
(k^3 * elements * 2 FLOP at 157.3 TFLOP/s).
usage: python tools/bench_dwconv_large.py [min_seconds]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from medicalsemseg_amd import hip

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
PEAK = 157.3e12
dev = torch.device("cuda:0")
dt = torch.bfloat16


def sample(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def alternate(fa, fb):
    """us per call of fa and fb (fb may be None), samples of about 5 ms alternating until each has WINDOW seconds on the device"""
    out = []
    reps = []
    for f in (fa, fb):
        if f is None:
            reps.append(0)
            continue
        f()
        torch.cuda.synchronize()
        t = sample(f, 1)                       # second call: warm
        reps.append(max(1, min(1000, int(5e-3 / max(t, 1e-6)))))
    tot, cnt = [0.0, 0.0], [0, 0]
    t0 = time.time()
    while any(r and tot[i] < WINDOW for i, r in enumerate(reps)) and time.time() - t0 < 60:
        for i, f in enumerate((fa, fb)):
            if reps[i] and tot[i] < WINDOW:
                tot[i] += sample(f, reps[i])
                cnt[i] += reps[i]
    for i in range(2):
        out.append(tot[i] / cnt[i] * 1e6 if cnt[i] else None)
    return out


def fmt(v):
    return "not measured" if v is None else f"{v:9.1f}"


print("    C   grid   K |      fwd (share of bound)     dgrad      wgrad |  stock fwd  stock dgrad  stock wgrad   (us per call)")
for C, e in ((48, 48), (96, 24), (192, 12), (384, 6)):
    for K in (9, 11):
        N = 2
        x = torch.randn(N, e, e, e, C, device=dev).to(dt)
        dy = torch.randn(N, e, e, e, C, device=dev).to(dt)
        w = torch.randn(C, 1, K, K, K, device=dev) * float(K) ** -1.5
        taps = w.reshape(C, -1).t().contiguous().to(dt)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        dw = torch.zeros_like(w)
        xa, dya, wa = x.permute(0, 4, 1, 2, 3), dy.permute(0, 4, 1, 2, 3), w.to(dt)    # NCDHW views of channels-last storage
        stock = [lambda: F.conv3d(xa, wa, None, padding=K // 2, groups=C),
                 lambda: torch.ops.aten.convolution_backward(dya, xa, wa, None, [1] * 3, [K // 2] * 3, [1] * 3, False, [0] * 3, C,
                                                             [True, False, False]),
                 lambda: torch.ops.aten.convolution_backward(dya, xa, wa, None, [1] * 3, [K // 2] * 3, [1] * 3, False, [0] * 3, C,
                                                             [False, True, False])]
        ours = [lambda: hip.dwconv3d(x, taps, y, K), lambda: hip.dwconv3d(dy, taps, dx, K, flip=True),
                lambda: hip.dwconv3d_wgrad(x, dy, dw, K)]
        res = []
        for fo, fs in zip(ours, stock):
            try:
                res.append(alternate(fo, fs))
            except RuntimeError as err:          # the stock path has no kernel for the shape
                print(f"# stock path failed at C {C} grid {e} K {K}: {str(err).splitlines()[0][:100]}")
                res.append([alternate(fo, None)[0], None])
        bound = K ** 3 * N * e ** 3 * C * 2 / PEAK * 1e6
        print(f"{C:5d} {e:3d}^3 {K:3d} | {res[0][0]:9.1f} ({100 * bound / res[0][0]:5.1f} % of {bound:6.1f}) {res[1][0]:9.1f}  {res[2][0]:9.1f} | "
              f"{fmt(res[0][1])}  {fmt(res[1][1])}  {fmt(res[2][1])}", flush=True)
