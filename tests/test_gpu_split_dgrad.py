"""Split output of the ping-pong conv k3 kernel (csrc/conv3d_k3_pp.hip, msseg_conv3d_k3_fwd_split): the output channels
[0, split) go to one tensor and [split, Cout) to another, so that the input gradient of a conv over cat([skip | up]) comes out
as two dense tensors.  Every element is computed by the same instructions from the same operands as in the one-output launch,
only its address differs: all comparisons are torch.equal against hip.conv3d_k3 into one Cout-wide buffer.

Shapes are the smallest the ping-pong kernel accepts, tiles * (Cout / 32) >= 2 * CUs with 4 x 4 x 16 tiles."""
import functools

import pytest
import torch

from tests.test_gpu_kernels import _dev

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENTINEL = -77.0            # exactly representable in bf16; conv outputs of the random operands below stay within +-10


@functools.lru_cache(maxsize=None)
def _case(vol, cout):
    """random bf16 operands of conv k3 32 -> cout on the grid vol and the one-output result (computed once per shape)"""
    from medicalsemseg_amd import hip
    dev = _dev()
    N, D, H, W = vol
    g = torch.Generator().manual_seed(7 + cout + D)
    x = torch.randn(N, D, H, W, 32, generator=g).to(dev, BF16)
    w = (torch.randn(cout, 32, 3, 3, 3, generator=g) * (27 * 32) ** -0.5).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    assert hip.lib().msseg_conv3d_k3_kernel(N, D, H, W, 32, cout, hip.BF16) == 3, "the shape must run on k3pp_kernel"
    wp = hip.pack_conv_k3(w, BF16, vol=vol)
    y = torch.full((N, D, H, W, cout), SENTINEL, dtype=BF16, device=dev)
    hip.conv3d_k3(x, wp, b, y, 32, cout)
    torch.cuda.synchronize()
    assert not bool((y == SENTINEL).any())
    return x, wp, b, y


@pytest.mark.parametrize("vol", [(2, 32, 32, 32),      # 256 full tiles: one tile per workgroup, prologue + last-phase epilogue only
                                 (2, 36, 34, 40)])     # partial tiles on every axis: the masked epilogue
def test_two_dense_halves_equal_the_one_output_launch(vol):
    from medicalsemseg_amd import hip
    x, wp, b, y = _case(vol, 64)
    assert hip.conv3d_k3_split_ok(vol, 32, 64, 32, BF16)
    ya = torch.full(vol + (32,), SENTINEL, dtype=BF16, device=x.device)
    yb = torch.full(vol + (32,), SENTINEL, dtype=BF16, device=x.device)
    hip.conv3d_k3_split(x, wp, b, ya, yb, 32, 64)
    torch.cuda.synchronize()
    assert torch.equal(ya, y[..., :32])
    assert torch.equal(yb, y[..., 32:])


@pytest.mark.parametrize("split", [64, 32])            # split_cb 2 and 1 of 4 cout blocks
def test_uneven_split_into_slices_of_wider_buffers(split):
    from medicalsemseg_amd import hip
    vol = (2, 32, 32, 32)
    x, wp, b, y = _case(vol, 128)
    assert hip.conv3d_k3_split_ok(vol, 32, 128, split, BF16)
    ca, cb = split, 128 - split
    bufa = torch.full(vol + (ca + 40,), SENTINEL, dtype=BF16, device=x.device)
    bufb = torch.full(vol + (cb + 24,), SENTINEL, dtype=BF16, device=x.device)
    ya, yb = bufa[..., 8:8 + ca], bufb[..., 16:16 + cb]
    hip.conv3d_k3_split(x, wp, b, ya, yb, 32, 128)
    torch.cuda.synchronize()
    assert torch.equal(ya, y[..., :split])
    assert torch.equal(yb, y[..., split:])
    for buf, lo, hi in ((bufa, 8, 8 + ca), (bufb, 16, 16 + cb)):
        assert bool((buf[..., :lo] == SENTINEL).all()) and bool((buf[..., hi:] == SENTINEL).all())


def test_rejections_launch_nothing():
    from medicalsemseg_amd import hip
    vol = (2, 32, 32, 32)
    x, wp, b, y = _case(vol, 64)
    dev = x.device
    ya = torch.full(vol + (32,), SENTINEL, dtype=BF16, device=dev)
    yb = torch.full(vol + (32,), SENTINEL, dtype=BF16, device=dev)
    stats = torch.full((2, 64, 2), SENTINEL, device=dev)
    with pytest.raises(hip.MssegError, match="plain epilogue"):
        hip.conv3d_k3_split(x, wp, b, ya, yb, 32, 64, stats=stats)
    with pytest.raises(hip.MssegError, match="plain epilogue"):
        hip.conv3d_k3_split(x, wp, b, ya, yb, 32, 64, accumulate=True)
    # a split off the 32-channel boundary
    assert not hip.conv3d_k3_split_ok(vol, 32, 64, 16, BF16) and not hip.conv3d_k3_split_ok(vol, 32, 64, 48, BF16)
    assert not hip.conv3d_k3_split_ok(vol, 32, 64, 0, BF16) and not hip.conv3d_k3_split_ok(vol, 32, 64, 64, BF16)
    y16 = torch.full(vol + (16,), SENTINEL, dtype=BF16, device=dev)
    y48 = torch.full(vol + (48,), SENTINEL, dtype=BF16, device=dev)
    with pytest.raises(hip.MssegError, match="32-channel boundary"):
        hip.conv3d_k3_split(x, wp, b, y16, y48, 32, 64)
    # a problem of the generic kernels (16^3)
    small = (2, 16, 16, 16)
    assert hip.lib().msseg_conv3d_k3_kernel(*small, 32, 64, hip.BF16) != 3
    assert not hip.conv3d_k3_split_ok(small, 32, 64, 32, BF16)
    xs = x[:, :16, :16, :16].contiguous()
    sa = torch.full(small + (32,), SENTINEL, dtype=BF16, device=dev)
    sb = torch.full(small + (32,), SENTINEL, dtype=BF16, device=dev)
    with pytest.raises(hip.MssegError, match="ping-pong"):
        hip.conv3d_k3_split(xs, wp, b, sa, sb, 32, 64)
    torch.cuda.synchronize()
    for t in (ya, yb, y16, y48, sa, sb, stats):
        assert bool((t == SENTINEL).all()), "a rejected call wrote to an output"


def _unet_step(monkeypatch, off):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models.unet import UNet
    dev = _dev()
    if off:
        monkeypatch.setenv("MSSEG_NO_SPLIT_DGRAD", "1")
    else:
        monkeypatch.delenv("MSSEG_NO_SPLIT_DGRAD", raising=False)
    calls = []
    real = hip.conv3d_k3_split
    monkeypatch.setattr(hip, "conv3d_k3_split", lambda *a, **k: (calls.append(tuple(a[0].shape[:4])), real(*a, **k))[1])
    torch.manual_seed(0)
    net = UNet(1, 3, compute_dtype=BF16).to(dev)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 1, 32, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 3, (2, 1, 32, 32, 32), generator=g).float().to(dev)
    loss = DiceCELoss()(net((x, None, None)), y)
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(hip, "conv3d_k3_split", real)
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters()}, calls


def test_unet_step_same_gradients_with_split_input_gradient(monkeypatch):
    """UNet(1, 3) in bf16, batch 2, 32^3, forward + DiceCE + backward: level 0 (32^3) takes the split output, level 1 (16^3)
    falls back to the two views of one tensor; the loss and every parameter gradient equal those of MSSEG_NO_SPLIT_DGRAD=1"""
    loss_on, g_on, calls_on = _unet_step(monkeypatch, False)
    loss_off, g_off, calls_off = _unet_step(monkeypatch, True)
    assert calls_on == [(2, 32, 32, 32)] and calls_off == [], (calls_on, calls_off)
    assert torch.equal(loss_on, loss_off)
    assert g_on.keys() == g_off.keys() and len(g_on) > 40
    for n in g_on:
        assert torch.equal(g_on[n], g_off[n]), f"gradient of {n} differs between the split and the one-tensor input gradient"
