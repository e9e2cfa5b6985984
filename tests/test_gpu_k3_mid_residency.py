"""The generic conv k3 kernel on 4x4x8 tiles (csrc/igemm_k3_mid.hip) with its statistics area sized by the launch's batch:
how many of its workgroups a CU holds, and that the re-laid-out area still gives exact outputs and sums.

References are exact: operands are small integers (tests/test_gpu_conv_exact.py, `ints`), so every product and every partial
sum in any order is an integer far below 2^24.  That also holds for the CPU reference itself when it is computed in fp32, which
is what `_ref` does (a 128-channel float64 convolution takes seconds on the CPU, the fp32 one milliseconds); `assert_exact`
then checks on the reference alone that it is integer-valued and within the exact range of the storage dtype.

InstanceNorm-backward sums (conv3d_k3_dgrad_inbwd): red[n][c] = (sum dz, rstd * (sum dz * yraw - mean * sum dz)) with
dz = da * (act > 0 ? 1 : slope).  The test passes forward statistics (0, S) of S voxels, eps = 3 and slope = 0.5: mean = 0,
var = fl(S * fl(1 / S)) is within one ulp of 1, var + eps rounds to 4 (asserted below in numpy's fp32), rstd = 0.5, and the
sums of half-integers stay exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_conv_exact import assert_exact, int_bias, ints, vol
from tests.test_gpu_kernels import _dev, cl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
COUT = 64
SWITCH = "MSSEG_K3_MID_ONE_PER_CU"
LEVEL = (2, 24, 24, 24, 64, COUT)       # the UNet's 24^3 level at batch 2


# ------------------------------------------------------------------------------------------------------------------
# residency
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("N", [2, 1, 4])
def test_two_workgroups_per_cu(N, dtype):
    from medicalsemseg_amd import hip
    _dev()
    assert hip.lib().msseg_conv3d_k3_kernel(N, 24, 24, 24, 64, COUT, hip._DT[dtype]) == 1      # the 4x4x8 tile
    got = hip.conv_k3_resident_per_cu(N, 24, 24, 24, 64, COUT, dtype)
    print(f"resident workgroups per CU, N={N} 24^3 64->64 {dtype}: {got}")
    assert got == 2


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_full_batch_still_resident(dtype):
    from medicalsemseg_amd import hip
    _dev()
    got = hip.conv_k3_resident_per_cu(8, 24, 24, 24, 64, COUT, dtype)
    print(f"resident workgroups per CU, N=8 24^3 64->64 {dtype}: {got}")
    assert got >= 1


# ------------------------------------------------------------------------------------------------------------------
# the switch, in a fresh process (the library reads it once)
# ------------------------------------------------------------------------------------------------------------------
def _level_case(dev):
    """random bf16 operands of the 24^3 level -> (output, fused statistics, residency in bf16 and f32), all on the CPU"""
    from medicalsemseg_amd import hip
    N, D, H, W, cin, cout = LEVEL
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, D, H, W, cin, generator=g).to(dev, BF16)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * (27 * cin) ** -0.5).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    assert hip.lib().msseg_conv3d_k3_kernel(N, D, H, W, cin, cout, hip.BF16) == 1
    y = torch.full((N, D, H, W, cout), float("nan"), dtype=BF16, device=dev)
    stats = torch.full((N, cout, 2), float("nan"), device=dev)
    hip.conv3d_k3(x, hip.pack_conv_k3(w, BF16, vol=(N, D, H, W)), b, y, cin, cout, stats)
    torch.cuda.synchronize()
    res = [hip.conv_k3_resident_per_cu(N, D, H, W, cin, cout, d) for d in (BF16, F32)]
    return dict(y=y.float().cpu(), stats=stats.cpu(), resident=res)


def _child(path):
    torch.save(_level_case(torch.device("cuda:0")), path)


@pytest.fixture(scope="module")
def one_per_cu(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("k3mid") / "one_per_cu.pt")
    r = subprocess.run([sys.executable, "-c", f"from tests.test_gpu_k3_mid_residency import _child; _child({path!r})"],
                       env=dict(os.environ, **{SWITCH: "1"}), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return torch.load(path, map_location="cpu", weights_only=True)


def test_switch_restores_one_workgroup_per_cu(one_per_cu):
    assert SWITCH not in os.environ, "the in-process cases of this file need the default residency"
    print(f"resident workgroups per CU with {SWITCH}=1 (bf16, f32): {one_per_cu['resident']}")
    assert one_per_cu["resident"] == [1, 1]


def test_same_bits_under_either_residency(one_per_cu):
    here = _level_case(_dev())
    assert here["resident"] == [2, 2]
    assert torch.equal(here["y"], one_per_cu["y"]), "outputs differ between one and two workgroups per CU"
    assert torch.equal(here["stats"], one_per_cu["stats"]), "fused statistics differ between one and two workgroups per CU"


# ------------------------------------------------------------------------------------------------------------------
# exact outputs and sums on the 4x4x8 tile
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _ref(cin, sp, N, thin=1, scale_samples=False):
    """x [N, cin, *sp], w [64, cin, 3, 3, 3], bias, y0 = conv(x, w) without bias; all float64 on the CPU, computed in fp32 (exact:
    see the module docstring).  thin: divides the operands' density; scale_samples: sample n is multiplied by n + 1."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    K = 27 * cin * thin * thin
    x = ints((N, cin, *sp), K, 1)
    if scale_samples:
        x = x * torch.arange(1, N + 1, dtype=torch.float64).view(N, 1, 1, 1, 1)
    w = ints((COUT, cin, 3, 3, 3), K, 2)
    y0 = F.conv3d(x.float(), w.float(), None, padding=1).double()
    return dict(x=x, w=w, b=int_bias(COUT, 3), y0=y0)


def _stats_ref(y64):
    f = y64.reshape(y64.shape[0], y64.shape[1], -1)
    s, s2 = f.sum(2), (f * f).sum(2)
    assert float(s2.max()) < 2 ** 24, "the reference sum of squares is not exact in fp32: lower the input density"
    return torch.stack([s, s2], -1)


def _planned_on_mid_tile(N, sp, cin, dtype):
    from medicalsemseg_amd import hip
    L = hip.lib()
    assert L.msseg_conv3d_k3_variant(N, *sp, COUT) == 1 and L.msseg_conv3d_k3_kernel(N, *sp, cin, COUT, hip._DT[dtype]) == 1
    assert L.msseg_conv3d_k3_cout_block(N, *sp, COUT) == 32


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cin", [32, 64, 128])
@pytest.mark.parametrize("sp", [(16, 16, 24), (14, 18, 20)])
def test_mid_tile_exact(sp, cin, dtype):
    """forward with fused statistics, plain forward, and the input-gradient launch with the InstanceNorm-backward sums"""
    from medicalsemseg_amd import hip
    dev, N = _dev(), 2
    _planned_on_mid_tile(N, sp, cin, dtype)
    r = _ref(cin, sp, N)
    y_ref = r["y0"] + r["b"].view(1, -1, 1, 1, 1)
    xg, w, b = cl(r["x"], dtype, dev), r["w"].float().to(dev), r["b"].float().to(dev)
    wp = hip.pack_conv_k3(w, dtype, vol=(N, *sp))

    y = torch.full((N, *sp, COUT), float("nan"), dtype=dtype, device=dev)
    stats = torch.full((N, COUT, 2), float("nan"), device=dev)
    hip.conv3d_k3(xg, wp, b, y, cin, COUT, stats)
    assert_exact(vol(y), y_ref, "forward with statistics")
    assert_exact(stats, _stats_ref(y_ref), "fused statistics")

    y = torch.full((N, *sp, COUT), float("nan"), dtype=dtype, device=dev)
    hip.conv3d_k3(xg, wp, b, y, cin, COUT)
    assert_exact(vol(y), y_ref, "plain forward")

    # input gradient of the layer v = w^T with flipped taps (cin gradient channels in, 64 out): da = conv(x, w)
    v = w.transpose(0, 1).flip(2, 3, 4).contiguous()
    S = sp[0] * sp[1] * sp[2]
    var = np.float32(S) * (np.float32(1) / np.float32(S))
    assert np.float32(var + np.float32(3.0)) == np.float32(4.0)
    g = torch.Generator().manual_seed(5)
    yraw = torch.randint(-1, 2, (N, COUT, *sp), generator=g).double()
    act = torch.randint(0, 2, (N, COUT, *sp), generator=g).double() * 2 - 1
    fwd_stats = torch.tensor([0.0, float(S)]).repeat(N, COUT, 1).to(dev)
    da = torch.full((N, *sp, COUT), float("nan"), dtype=dtype, device=dev)
    dgamma, dbeta = torch.full((COUT,), float("nan"), device=dev), torch.full((COUT,), float("nan"), device=dev)
    red = hip.conv3d_k3_dgrad_inbwd(xg, hip.pack_conv_k3(v, dtype, dgrad=True, vol=(N, *sp)), da, cin, COUT, cl(yraw, dtype, dev),
                                    cl(act, dtype, dev), fwd_stats, 0.5, 3.0, dgamma, dbeta)
    assert_exact(vol(da), r["y0"], "input gradient")
    dz = r["y0"] * torch.where(act > 0, 1.0, 0.5)
    red_ref = torch.stack([dz.sum((2, 3, 4)), 0.5 * (dz * yraw).sum((2, 3, 4))], -1)
    # multiples of 1/4 (slope and rstd are 1/2) below 2^22: exact in fp32 in any summation order
    assert bool((4 * red_ref == (4 * red_ref).round()).all()) and float(red_ref.abs().max()) < 2 ** 22
    assert torch.equal(red.double().cpu(), red_ref), "InstanceNorm-backward sums"
    assert torch.equal(dbeta.double().cpu(), red_ref[..., 0].sum(0)) and torch.equal(dgamma.double().cpu(), red_ref[..., 1].sum(0))


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("N", [1, 3, 6, 7, 8])
def test_sample_slots_exact(N, dtype):
    """32 -> 64 at 16 x 16 x 24 with sample n multiplied by n + 1: a slot mix-up changes the sums.  N = 1 is planned on the 2x4x8
    tile and bf16 N = 8 on the ping-pong kernel (printed); every other case runs the 4x4x8 tile, N = 8 in fp32 with all slots"""
    from medicalsemseg_amd import hip
    dev, sp, cin = _dev(), (16, 16, 24), 32
    kern = hip.lib().msseg_conv3d_k3_kernel(N, *sp, cin, COUT, hip._DT[dtype])
    print(f"sample slots N={N} {dtype}: kernel {kern}, resident per CU "
          f"{hip.conv_k3_resident_per_cu(N, *sp, cin, COUT, dtype) if kern <= 2 else 'n/a'}")
    assert kern == (2 if N == 1 else 3 if (N == 8 and dtype == BF16) else 1) or hip.lib().msseg_num_cus() != 256
    r = _ref(cin, sp, N, thin=8, scale_samples=True)
    y_ref = r["y0"] + r["b"].view(1, -1, 1, 1, 1)
    y = torch.full((N, *sp, COUT), float("nan"), dtype=dtype, device=dev)
    stats = torch.full((N, COUT, 2), float("nan"), device=dev)
    hip.conv3d_k3(cl(r["x"], dtype, dev), hip.pack_conv_k3(r["w"].float().to(dev), dtype, vol=(N, *sp)), r["b"].float().to(dev), y,
                  cin, COUT, stats)
    assert_exact(vol(y), y_ref, "forward with statistics")
    ref = _stats_ref(y_ref)
    assert len({tuple(ref[n, :, 0].tolist()) for n in range(N)}) == N, "two samples share their sums: the case proves nothing"
    assert_exact(stats, ref, "fused statistics per sample")
