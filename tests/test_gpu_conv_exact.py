"""Bit-exact tests of the convolution family on integer inputs.

Every operand is in {-1, 0, +1} (exact in bf16 and fp32) and sparse enough that every output is an integer with |y| <= 256
(exact in bf16; fp32 outputs: < 2^24).  Then every product, every partial sum in any order and the stored result are exact,
and a kernel must EQUAL the float64 CPU reference whatever its tiling, split-K or summation order: one wrong halo tap at one
voxel fails `torch.equal`, where the relative gates of tests/test_gpu_kernels.py (6e-3 of the output's maximum in bf16) let it
pass (tests/test_conv_exact_method.py shows both on the CPU).  DESIGN.md, "Exact integer-input tests", lists kernel -> case.

Every case prints the kernel or path that took it and asserts it wherever the library has a query for it.

Instantiations of the generic kernel (csrc/igemm_fwd_kernel.h) and the case that runs each, in fp32 and in bf16 unless noted;
"cout block" is the kernel's NT * 16, dgrad the input gradient of a case (cout -> cin channels):
  igemm_k3_small.hip (2x4x8)   16: test_conv3d_k3_exact 8->24 @5x7x9, 128->256 @6^3, 160->32 @8^3;  32: dgrad of 64->144 @7x9x11;
                               48: 64->144 @7x9x11
  igemm_k3_mid.hip (4x4x8)     16: 24->16 @13x15x17;  32: 72->32 @13x12x14, dgrad of 24->16;  48: 48->48 @12x12x24
  igemm_k3_big_*.hip (4x8x16)  16: dgrad of 16->48 @32x33x34;  32: 16->48 @32x33x34 (Cout = 48 on two 32-wide blocks), fp32 32->32
                               @32x33x34, bf16 64->32 @34x33x50;  no 48-wide instantiation (IGEMM_K3)
  igemm_k3s2.hip               16: test_conv3d_k3s2_exact 16->16 @5x6x7;  32: the four S2_CASES;  48: 16->48 @5x6x7
  igemm_flat.hip, direct       fp32: test_linear_exact 1152->16 (16), 3072->768 and every dgrad but the last (32), 1536->48, 48->144
                               (48);  bf16: the 301-token cases 32->16 (16), 128->32 (32), 32->48 (48)
  igemm_flat.hip, gather       test_conv3d_gather_exact 4->16 (16), 4->32 and 1->32 k7 (32), 1->48 k2 (48)
  igemm_flat.hip, deconv       32 only: test_deconv_k2s2_exact, fp32 every case, bf16 the Cout = 8 cases
  igemm_flat.hip, deconv_bwd   cout block of Cin: fp32 16->8 (16), 48->48 (48), the others (32);  bf16 16->8, 32->8, 48->8"""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_kernels import _dev, check, cl, gen, ncdhw, rnd

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
TILE = (4, 4, 16)        # tile of the ping-pong / 48-channel / stem kernels: where a tile-edge predicate goes wrong


# ------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------
def ints(shape, K, seed):
    """CPU float64 tensor of +-1 signs under a Bernoulli mask of density min(1, 24 / sqrt(K)); K = the contraction length of the op
    that consumes the tensor.  A sum of K products of two such tensors has a standard deviation of at most 24: |y| <= 256 is
    more than ten of them away."""
    g = torch.Generator().manual_seed(seed)
    shape = tuple(shape)
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    keep = torch.rand(shape, generator=g, dtype=torch.float64) < min(1.0, 24.0 / K ** 0.5)
    return sign * keep


def int_bias(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (n,), generator=g).double()


def assert_exact(got, ref64, what):
    """got == ref64 bit for bit.  First the conditions, on the reference alone, that make exactness legitimate: integer values,
    |ref| <= 256 where the result is stored in bf16 (any `got` that is not fp32), < 2^24 for fp32 results.  If a new shape breaks
    them, lower the density of its inputs: the comparison stays an equality."""
    assert ref64.dtype == torch.float64 and not ref64.is_cuda
    assert bool((ref64 == ref64.round()).all()), f"{what}: the reference is not integer-valued"
    top = float(ref64.abs().max())
    if got.dtype == torch.float32:
        assert top < 2 ** 24, f"{what}: reference maximum {top} is not exact in fp32 sums"
    else:
        assert top <= 256, f"{what}: reference maximum {top} is not exact in bf16: lower the input density"
    g = got.detach().double().cpu()
    assert g.shape == ref64.shape, f"{what}: shape {tuple(g.shape)} vs reference {tuple(ref64.shape)}"
    if torch.equal(g, ref64):
        return
    bad = (g != ref64).nonzero()
    msg = f"{what}: {bad.shape[0]} of {g.numel()} elements differ; first (index: got, want): "
    msg += ", ".join(f"{tuple(i.tolist())}: {float(g[tuple(i)])}, {float(ref64[tuple(i)])}" for i in bad[:6])
    if g.dim() == 5:     # (n, c, z, y, x): is every mismatch on a volume face / on the first or last voxel of a 4x4x16 tile?
        zyx, ext = bad[:, 2:], torch.tensor(g.shape[2:])
        face = ((zyx == 0) | (zyx == ext - 1)).any(1)
        t = torch.tensor(TILE)
        edge = ((zyx % t == 0) | (zyx % t == t - 1)).any(1)
        msg += f"; all on a volume face: {bool(face.all())}; all on a {TILE} tile edge: {bool(edge.all())}"
    raise AssertionError(msg)


def vol(t):
    """channels-last [N, D, H, W, C] -> (n, c, z, y, x) view, dtype kept (assert_exact reads the storage dtype off it)"""
    return t.permute(0, 4, 1, 2, 3)


class launched:
    """names of the main kernels launched inside the block, from the library's own per-launch records (msseg_ktimer_*): the
    path report for ops without a query function"""

    def __enter__(self):
        from medicalsemseg_amd import hip
        hip.ktimer_enable(True)
        hip.load_library().msseg_ktimer_reset()
        self.names = set()
        return self

    def __exit__(self, *exc):
        from medicalsemseg_amd import hip
        try:
            if exc[0] is None:
                self.names = set(hip.ktimer_summary())
        finally:
            hip.ktimer_enable(False)
            hip.load_library().msseg_ktimer_reset()


def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _grow_n(n0, ok, what, nmax=32):
    """smallest N >= n0 for which the eligibility rule (tile counts against the card's CU count) selects the wanted kernel"""
    for n in range(n0, nmax + 1):
        if ok(n):
            return n
    pytest.fail(f"{what}: no batch size in {n0} ... {nmax} selects the kernel on this card")


def _sumsq_err(stats, y64):
    """(exactness of the sums is asserted, relative error of the sums of squares is returned); y64: (n, c, z, y, x)"""
    N, C = y64.shape[:2]
    f = y64.reshape(N, C, -1)
    assert_exact(stats[..., 0], f.sum(2), "fused statistics: sum")
    ref = (f * f).sum(2)
    return float((stats[..., 1].double().cpu() - ref).abs().max() / ref.abs().max())


# Relative error of the fused sum of squares against float64.  Below 2^24 (every grid here up to 12 x 12 x 24, and the stem cases:
# |y| <= 30 over at most 8190 voxels) the fp32 sums are exact and the measured error is 0; above it (fp32 accumulation of positive
# terms) the gate is 4 x the largest value measured on an MI355X, far below the 1e-5 of tests/test_gpu_kernels.py.
SUMSQ_GATES = {
    "k3": 6.2e-7,      # measured 1.440e-07 (fp32 32->32 @32x33x34), 1.534e-07 (64->32 @34x33x50), 1.133e-07 / 1.130e-07 (ping-pong
                       # 32->32 / 32->64 @30x29x70), 1.467e-07 (48->48 @30x33x36), 1.458e-07 (96->48 as halves), 0 on all others
    "stem": 0.0,       # measured 0 on both cases: exact (asserted with <=)
}


# ------------------------------------------------------------------------------------------------------------------
# conv 3x3x3 s1 p1: forward, input gradient, weight gradient, bias gradient through layers.Conv3
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _k3_ref(cin, cout, sp, N, stride=1):
    _threads()
    x = ints((N, cin, *sp), 27 * cin, 1).requires_grad_(True)
    w = ints((cout, cin, 3, 3, 3), 27 * cin, 2).requires_grad_(True)
    b = int_bias(cout, 3)
    y = F.conv3d(x, w, b, stride=stride, padding=1)
    dy = ints(y.shape, 27 * cout, 4)
    y.backward(dy)
    return dict(x=x.detach(), w=w.detach(), b=b, dy=dy, y=y.detach(), dx=x.grad, dw=w.grad, db=dy.sum((0, 2, 3, 4)))


# (cin, cout, grid, first N, dtype, forward kernel [msseg_conv3d_k3_kernel: 0 / 1 / 2 = generic igemm on 4x8x16 / 4x4x8 / 2x4x8
# tiles, 3 = ping-pong, 4 = 48-channel], weight-gradient kernel [msseg_conv3d_k3_wgrad_kernel: 3 = ping-pong, 0 = generic; None:
# reported only]).  N grows from the listed value until the card's CU count selects the kernel.
K3_CASES = [
    # generic igemm, 2x4x8 tiles
    (8, 24, (5, 7, 9), 2, F32, 2, 0), (8, 24, (5, 7, 9), 2, BF16, 2, None),
    (128, 256, (6, 6, 6), 2, F32, 2, 0), (128, 256, (6, 6, 6), 2, BF16, 2, None),
    (160, 32, (8, 8, 8), 2, F32, 2, 0), (160, 32, (8, 8, 8), 2, BF16, 2, None),     # odd block count, partial last block
    # generic igemm, 4x4x8 tiles
    (48, 48, (12, 12, 24), 2, F32, 1, 0), (48, 48, (12, 12, 24), 2, BF16, 1, None),
    (72, 32, (13, 12, 14), 2, F32, 1, 0), (72, 32, (13, 12, 14), 2, BF16, 1, None),
    # generic igemm, 4x8x16 tiles; bf16 with two channel blocks per stage
    (32, 32, (32, 33, 34), 2, F32, 0, 0),
    (64, 32, (34, 33, 50), 2, BF16, 0, 3),
    # ping-pong forward (and input gradient of 32 -> 32: 32 gradient channels in) + ping-pong weight gradient
    (32, 32, (30, 29, 70), 2, BF16, 3, 3),
    (32, 64, (30, 29, 70), 2, BF16, 3, 3),
    # 48-channel kernel (forward and input gradient: 48 gradient channels in)
    (48, 48, (30, 33, 36), 3, BF16, 4, 3),
    # generic igemm, the (tile, cout block) pairs the generic cases above leave out (IGEMM_K3 below): 2x4x8 with 48- (forward) and 32-wide
    # (input gradient) blocks; 4x4x8 with 16-wide blocks; 4x8x16 with Cout = 48 on 32-wide blocks, the second half empty (forward),
    # and with 16-wide blocks (input gradient).  Odd extents: partial tiles on every axis of the two smaller tiles.
    (64, 144, (7, 9, 11), 4, F32, 2, 0), (64, 144, (7, 9, 11), 4, BF16, 2, None),
    (24, 16, (13, 15, 17), 2, F32, 1, 0), (24, 16, (13, 15, 17), 2, BF16, 1, None),
    (16, 48, (32, 33, 34), 2, F32, 0, 0), (16, 48, (32, 33, 34), 2, BF16, 0, None),
]


# What the generic cases run of igemm_fwd_kernel<27 taps, stride 1> on a card with 256 CUs (k3_plan counts workgroups against
# 3/4 of them): (cin, cout, grid) -> (forward cout block, input-gradient kernel, input-gradient cout block), the same for both
# dtypes unless a bf16 row says otherwise.  Every reachable (tile, cout block) pair of csrc/igemm_k3_{small,mid,big}.hip is here
# in fp32 and bf16; the 4x8x16 tile has no 48-wide block (k3_plan answers 32).
IGEMM_K3 = {
    (8, 24, (5, 7, 9)): (16, 2, 16), (128, 256, (6, 6, 6)): (16, 2, 16), (160, 32, (8, 8, 8)): (16, 2, 16),
    (64, 144, (7, 9, 11)): (48, 2, 32),
    (48, 48, (12, 12, 24)): (48, 1, 48), (72, 32, (13, 12, 14)): (32, 1, 32), (24, 16, (13, 15, 17)): (16, 1, 32),
    (32, 32, (32, 33, 34)): (32, 0, 32), (16, 48, (32, 33, 34)): (32, 0, 16),
    (64, 32, (34, 33, 50), BF16): (32, 3, 32),      # input gradient 32 -> 64 on the ping-pong kernel
}


@pytest.mark.parametrize("cin,cout,sp,n0,dtype,kern,wgk", K3_CASES)
def test_conv3d_k3_exact(cin, cout, sp, n0, dtype, kern, wgk):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.layers import Conv3
    dev = _dev()
    L, code = hip.lib(), hip._DT[dtype]
    N = _grow_n(n0, lambda n: L.msseg_conv3d_k3_kernel(n, *sp, cin, cout, code) == kern, f"conv {cin}->{cout} @ {sp} kernel {kern}")
    assert L.msseg_conv3d_k3_kernel(N, *sp, cin, cout, code) == kern
    if kern <= 2:
        assert L.msseg_conv3d_k3_variant(N, *sp, cout) == kern
    dgk = L.msseg_conv3d_k3_kernel(N, *sp, cout, cin, code)
    wg = L.msseg_conv3d_k3_wgrad_kernel(N, *sp, cin, cout, code)
    blocks = IGEMM_K3.get((cin, cout, sp, dtype), IGEMM_K3.get((cin, cout, sp)))
    assert (blocks is not None) == (kern <= 2)
    if blocks is not None and L.msseg_num_cus() == 256:
        assert (L.msseg_conv3d_k3_cout_block(N, *sp, cout), dgk, L.msseg_conv3d_k3_cout_block(N, *sp, cin)) == blocks
    if kern in (3, 4) and cin == cout:
        assert dgk == kern
    if wgk is not None:
        assert wg == wgk
    r = _k3_ref(cin, cout, sp, N)
    op = Conv3(torch.nn.Parameter(r["w"].float().to(dev)), torch.nn.Parameter(r["b"].float().to(dev)))
    xg, dyg = cl(r["x"], dtype, dev), cl(r["dy"], dtype, dev)
    small = hip.conv3d_k3_small_ok(dyg, cout, cin)
    with launched() as k:
        y = op.fwd(xg)
        dx = op.bwd(xg, dyg, True)
        dw1, db1 = op.w.grad.clone(), op.b.grad.clone()
        op.bwd(xg, dyg, False)
    print(f"conv3d_k3 {cin}->{cout} @ {sp} N={N} {dtype}: fwd kernel {kern} (cout block {L.msseg_conv3d_k3_cout_block(N, *sp, cout)}), "
          f"dgrad kernel {dgk}{' (split-K small grid)' if small else ''}, wgrad kernel {wg}; launched {sorted(k.names)}")
    assert ("k3pp_kernel" in k.names) == (kern == 3 or dgk == 3) and ("k3c48_kernel" in k.names) == (kern == 4 or dgk == 4)
    assert ("k3wg_pp_kernel" in k.names) == (wg == 3) and ("k3s_kernel" in k.names) == small
    assert_exact(vol(y), r["y"], "conv3d_k3 fwd")
    assert_exact(vol(dx), r["dx"], "conv3d_k3 dgrad")
    assert_exact(dw1, r["dw"], "conv3d_k3 wgrad")
    assert_exact(db1, r["db"], "conv3d_k3 bias grad")
    assert_exact(op.w.grad, 2 * r["dw"], "conv3d_k3 wgrad accumulate")
    assert_exact(op.b.grad, 2 * r["db"], "conv3d_k3 bias grad accumulate")
    if N <= 8:      # the same forward with the InstanceNorm statistics fused into the epilogue
        y2, stats = op.fwd(xg, want_stats=True)
        assert_exact(vol(y2), r["y"], "conv3d_k3 fwd with statistics")
        err = _sumsq_err(stats, r["y"])
        print(f"  fused sum of squares: relative error {err:.3e} (gate {SUMSQ_GATES['k3']:.1e})")
        assert err < SUMSQ_GATES["k3"]


def test_conv3d_k3_c48_smallest_grid_exact():
    """48 -> 16 (one 16-wide cout block) on the smallest cube, one voxel past a tile multiple on every axis, that the 48-channel
    kernel takes with N = 4"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.layers import Conv3
    dev, L = _dev(), hip.lib()
    N, cin, cout = 4, 48, 16
    s = next((s for s in range(9, 80, 4) if L.msseg_conv3d_k3_kernel(N, s, s, s, cin, cout, hip.BF16) == 4), None)
    assert s is not None, "no cube up to 77^3 selects the 48-channel kernel"
    sp = (s, s, s)
    assert L.msseg_conv3d_k3_kernel(N, s - 4, s, s, cin, cout, hip.BF16) != 4 or L.msseg_conv3d_k3_kernel(N, s, s, s - 16, cin, cout, hip.BF16) != 4
    r = _k3_ref(cin, cout, sp, N)
    op = Conv3(torch.nn.Parameter(r["w"].float().to(dev)), torch.nn.Parameter(r["b"].float().to(dev)))
    with launched() as k:
        y, stats = op.fwd(cl(r["x"], BF16, dev), want_stats=True)
    print(f"conv3d_k3 48->16 @ {sp} N={N}: launched {sorted(k.names)}")
    assert k.names == {"k3c48_kernel"}
    assert_exact(vol(y), r["y"], "conv 48 -> 16 fwd")
    err = _sumsq_err(stats, r["y"])
    print(f"  fused sum of squares: relative error {err:.3e}")
    assert err < SUMSQ_GATES["k3"]


def test_conv3d_k3_96_channels_two_accumulating_launches_exact():
    """96 -> 48 through Conv3.fwd(want_stats=True): two launches of the 48-channel kernel, the second accumulating onto the
    stored bf16 result of the first (an integer, so the extra rounding is exact too) and emitting the statistics"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.layers import Conv3
    dev, L = _dev(), hip.lib()
    cin, cout, sp, N = 96, 48, (30, 33, 36), 3
    r = _k3_ref(cin, cout, sp, N)
    op = Conv3(torch.nn.Parameter(r["w"].float().to(dev)), torch.nn.Parameter(r["b"].float().to(dev)))
    assert op.halves_ok((N, *sp), BF16) == 48
    xg, dyg = cl(r["x"], BF16, dev), cl(r["dy"], BF16, dev)
    with launched() as k:
        y, stats = op.fwd(xg, want_stats=True)
    print(f"conv3d_k3 96->48 @ {sp} N={N} as halves: launched {sorted(k.names)}")
    assert k.names == {"k3c48_kernel"}
    assert_exact(vol(y), r["y"], "conv 96 -> 48 as two halves")
    err = _sumsq_err(stats, r["y"])
    print(f"  fused sum of squares: relative error {err:.3e}")
    assert err < SUMSQ_GATES["k3"]
    # the layer's backward: input gradient on the 48-channel kernel (48 gradient channels in), ping-pong weight gradient
    assert L.msseg_conv3d_k3_kernel(N, *sp, cout, cin, hip.BF16) == 4 and L.msseg_conv3d_k3_wgrad_kernel(N, *sp, cin, cout, hip.BF16) == 3
    dx = op.bwd(xg, dyg, True)
    assert_exact(vol(dx), r["dx"], "conv 96 -> 48 dgrad")
    assert_exact(op.w.grad, r["dw"], "conv 96 -> 48 wgrad")


def test_conv3d_k3_64_channels_two_accumulating_launches_exact():
    """64 -> 32 through Conv3.fwd_split on the two 32-channel halves of the input: two launches of the ping-pong kernel, the
    second (csrc/conv3d_k3_pp.hip, STATS == 3) accumulating onto the stored bf16 result of the first and emitting the statistics.
    The first launch's stored intermediate is a partial sum of the same products: an integer, asserted here to stay within
    256, so the extra rounding is exact too."""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.layers import Conv3
    dev, L = _dev(), hip.lib()
    cin, cout, sp = 64, 32, (30, 29, 70)
    N = _grow_n(2, lambda n: L.msseg_conv3d_k3_kernel(n, *sp, 32, cout, hip.BF16) == 3, f"ping-pong 32->{cout} @ {sp}")
    assert L.msseg_conv3d_k3_kernel(N, *sp, 32, cout, hip.BF16) == 3
    r = _k3_ref(cin, cout, sp, N)
    part = F.conv3d(r["x"][:, :32], r["w"][:, :32], r["b"], padding=1)
    assert bool((part == part.round()).all()) and float(part.abs().max()) <= 256, "the first half's partial sum is not exact in bf16"
    op = Conv3(torch.nn.Parameter(r["w"].float().to(dev)), torch.nn.Parameter(r["b"].float().to(dev)))
    xg = cl(r["x"], BF16, dev)
    xa, xb = xg[..., :32].contiguous(), xg[..., 32:].contiguous()
    with launched() as k:
        y, stats = op.fwd_split(xa, xb)
    print(f"conv3d_k3 64->32 @ {sp} N={N} as halves: first half max |y| {float(part.abs().max()):.0f}, launched {sorted(k.names)}")
    assert k.names == {"k3pp_kernel"}
    assert_exact(vol(y), r["y"], "conv 64 -> 32 as two halves")
    err = _sumsq_err(stats, r["y"])
    print(f"  fused sum of squares: relative error {err:.3e}")
    assert err < SUMSQ_GATES["k3"]


@pytest.mark.parametrize("sp,want", [((8, 9, 17), 3), ((7, 9, 17), 0)])
def test_conv3d_k3_wgrad_pingpong_min_dim_cut_exact(sp, want):
    """64 -> 32 with enough samples that the tile count admits the ping-pong weight gradient: 8 x 9 x 17 takes it, 7 x 9 x 17 (the
    same tile count) falls to the generic kernel at the 8-voxel cut"""
    from medicalsemseg_amd import hip
    dev, L = _dev(), hip.lib()
    cin, cout = 64, 32
    N = _grow_n(2, lambda n: L.msseg_conv3d_k3_wgrad_kernel(n, 8, 9, 17, cin, cout, hip.BF16) == 3, "ping-pong wgrad 64->32 @ 8x9x17", 64)
    assert L.msseg_conv3d_k3_wgrad_kernel(N, *sp, cin, cout, hip.BF16) == want
    r = _k3_ref(cin, cout, sp, N)
    xg, dyg = cl(r["x"], BF16, dev), cl(r["dy"], BF16, dev)
    dw = torch.full((cout, cin, 3, 3, 3), float("nan"), device=dev)
    with launched() as k:
        hip.conv3d_k3_wgrad(xg, dyg, dw, cin, cout)
    print(f"conv3d_k3_wgrad 64->32 @ {sp} N={N}: launched {sorted(k.names)}")
    assert k.names == ({"k3wg_pp_kernel"} if want == 3 else {"igemm_wgrad_kernel<27>"})
    assert_exact(dw, r["dw"], "wgrad")
    hip.conv3d_k3_wgrad(xg, dyg, dw, cin, cout, True)
    assert_exact(dw, 2 * r["dw"], "wgrad accumulate")


@pytest.mark.parametrize("cin,cout,sp,N", [(64, 64, (3, 3, 3), 2), (128, 64, (6, 6, 6), 2), (96, 32, (12, 12, 12), 2),
                                           (768, 768, (3, 3, 3), 2)])
def test_conv3d_k3_small_grid_split_k_exact(cin, cout, sp, N):
    """split-K partials + the finish kernel as a plain sum of the stage groups: forward image (y without bias) and input-gradient
    image (dx), the shapes of test_resblock_small_grid_forward_backward"""
    from medicalsemseg_amd import hip
    dev = _dev()
    r = _k3_ref(cin, cout, sp, N)
    xg, dyg = cl(r["x"], BF16, dev), cl(r["dy"], BF16, dev)
    assert hip.conv3d_k3_small_ok(xg, cin, cout) and hip.conv3d_k3_small_ok(dyg, cout, cin)
    w = r["w"].float().to(dev)
    with launched() as k:
        part, ng = hip.conv3d_k3_small_partials(xg, hip.pack_conv_k3(w, BF16, cb=32), cin, cout)
        y = hip.conv3d_k3_small_bwd_finish(part, ng, torch.empty(N, *sp, cout, dtype=BF16, device=dev), unit=None)
        part, ngd = hip.conv3d_k3_small_partials(dyg, hip.pack_conv_k3(w, BF16, dgrad=True, cb=32), cout, cin)
        dx = hip.conv3d_k3_small_bwd_finish(part, ngd, torch.empty(N, *sp, cin, dtype=BF16, device=dev), unit=None)
    print(f"conv3d_k3_small {cin}->{cout} @ {sp} N={N}: stage groups fwd {ng}, dgrad {ngd}; launched {sorted(k.names)}")
    assert k.names == {"k3s_kernel"}
    if (cin, sp) in ((128, (6, 6, 6)), (768, (3, 3, 3))):
        assert ng >= 2 and ngd >= 2          # the sum over stage groups is really exercised
    assert_exact(vol(y), r["y"] - r["b"].view(1, -1, 1, 1, 1), "small-grid partials + finish, forward image")
    assert_exact(vol(dx), r["dx"], "small-grid partials + finish, input-gradient image")


@pytest.mark.parametrize("sp,N,kern", [((8, 8, 16), 1, 2), ((30, 29, 70), 2, 3)])
def test_conv3d_k3_channel_slices_exact(sp, N, kern):
    """input and output as channel slices of wider (concat) buffers, on the generic and on the ping-pong kernel; the untouched
    output channels keep their sentinel"""
    from medicalsemseg_amd import hip
    dev, L = _dev(), hip.lib()
    cin, cout = 32, (16 if kern == 2 else 32)
    N = _grow_n(N, lambda n: L.msseg_conv3d_k3_kernel(n, *sp, cin, cout, hip.BF16) == kern, f"conv slices @ {sp}")
    r = _k3_ref(cin, cout, sp, N)
    big_in = torch.zeros(N, *sp, 64, dtype=BF16, device=dev)
    big_in[..., 32:] = cl(r["x"], BF16, dev)
    big_in[..., :32] = 1.0                      # the neighbouring channels are not zero: a wrong channel offset shows
    big_out = torch.full((N, *sp, 16 + cout + 16), 7.0, dtype=BF16, device=dev)
    wp = hip.pack_conv_k3(r["w"].float().to(dev), BF16, vol=(N, *sp))
    with launched() as k:
        hip.conv3d_k3(big_in[..., 32:], wp, r["b"].float().to(dev), big_out[..., 16:16 + cout], cin, cout)
    print(f"conv3d_k3 slices 32->{cout} @ {sp} N={N}: launched {sorted(k.names)}")
    assert ("k3pp_kernel" in k.names) == (kern == 3)
    assert_exact(vol(big_out[..., 16:16 + cout]), r["y"], "conv into a channel slice")
    assert bool((big_out[..., :16] == 7.0).all()) and bool((big_out[..., 16 + cout:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------
# conv 3x3x3 stride 2 (igemm_fwd_kernel<STRIDE = 2>), zero_stuff2, ops.Conv3Fn stride-2 backward
# ------------------------------------------------------------------------------------------------------------------
S2_CASES = [(48, 96, (12, 12, 12)), (32, 64, (9, 10, 11)), (96, 192, (5, 6, 7)), (16, 32, (3, 3, 3))]
S2_PARAMS = [(*c, d) for c in S2_CASES for d in (F32, BF16)]
# the cases above have Cout % 32 == 0 (32-wide cout blocks of csrc/igemm_k3s2.hip): 16- and 48-wide blocks, odd extents
S2_EXACT_PARAMS = S2_PARAMS + [(*c, d) for c in [(16, 16, (5, 6, 7)), (16, 48, (5, 6, 7))] for d in (F32, BF16)]


def _s2_run(x, w, b, dy, dtype, dev):
    """(y of the kernel, zero-stuffed dy, y / dx / dW / db through ops.Conv3Fn) for NCDHW CPU operands"""
    from medicalsemseg_amd import hip, ops
    cout, cin = w.shape[:2]
    N = x.shape[0]
    xg, dyg = cl(x, dtype, dev), cl(dy, dtype, dev)
    y = torch.empty(N, *dy.shape[2:], cout, dtype=dtype, device=dev)
    hip.conv3d_k3s2(xg, hip.pack_conv_k3(w.float().to(dev), dtype), b.float().to(dev), y, cin, cout)
    dyz = torch.full((N, *x.shape[2:], cout), float("nan"), dtype=dtype, device=dev)
    hip.zero_stuff2(dyg, dyz)
    wp, bp = torch.nn.Parameter(w.float().to(dev)), torch.nn.Parameter(b.float().to(dev))
    xa = xg.clone().requires_grad_(True)
    ya = ops.Conv3Fn.apply(xa, wp, bp, 2)
    ya.backward(dyg)
    return y, dyz, ya.detach(), xa.grad, wp.grad, bp.grad


@pytest.mark.parametrize("cin,cout,sp,dtype", S2_EXACT_PARAMS)
def test_conv3d_k3s2_exact(cin, cout, sp, dtype):
    from medicalsemseg_amd import hip
    dev = _dev()
    assert hip.lib().msseg_cout_block(cout) == {16: 16, 32: 32, 48: 48, 64: 32, 96: 32, 192: 32}[cout]
    r = _k3_ref(cin, cout, sp, 2, 2)
    assert tuple(r["y"].shape[2:]) == tuple((v - 1) // 2 + 1 for v in sp)
    with launched() as k:
        y, dyz, ya, dx, dw, db = _s2_run(r["x"], r["w"], r["b"], r["dy"], dtype, dev)
    print(f"conv3d_k3s2 {cin}->{cout} @ {sp} {dtype}: launched {sorted(k.names)}")
    assert "igemm_fwd_kernel<27,2x4x8>" in k.names
    assert_exact(vol(y), r["y"], "conv3d_k3s2 fwd")
    assert_exact(vol(ya), r["y"], "Conv3Fn stride 2 fwd")
    stuffed = torch.zeros(2, cout, *sp, dtype=torch.float64)
    stuffed[:, :, ::2, ::2, ::2] = r["dy"]
    assert_exact(vol(dyz), stuffed, "zero_stuff2")
    assert_exact(vol(dx), r["dx"], "Conv3Fn stride 2 dgrad")
    assert_exact(dw, r["dw"], "Conv3Fn stride 2 wgrad")
    assert_exact(db, r["db"], "Conv3Fn stride 2 bias grad")


@pytest.mark.parametrize("cin,cout,sp,dtype", S2_PARAMS)
def test_conv3d_k3s2_randn(cin, cout, sp, dtype):
    """the stride-2 path on ordinary data at the suite's tolerances (the baseline coverage stride 1 has)"""
    dev = _dev()
    N = 2
    x = gen(N, cin, *sp, seed=1)
    w = gen(cout, cin, 3, 3, 3, seed=2, scale=(cin * 27) ** -0.5)
    b = gen(cout, seed=3)
    xr, wr = rnd(dtype, x, w)
    xr = xr.clone().requires_grad_(True)
    wr = wr.clone().requires_grad_(True)
    yref = F.conv3d(xr, wr, b, stride=2, padding=1)
    dy = gen(*yref.shape, seed=4)
    dyr = rnd(dtype, dy)
    yref.backward(dyr)
    y, dyz, ya, dx, dw, db = _s2_run(x, w, b, dy, dtype, dev)
    check(ncdhw(y), yref.detach(), dtype, "conv3d_k3s2 fwd")
    check(ncdhw(ya), yref.detach(), dtype, "Conv3Fn stride 2 fwd")
    stuffed = torch.zeros(N, cout, *sp)
    stuffed[:, :, ::2, ::2, ::2] = dyr
    assert torch.equal(ncdhw(dyz), stuffed)
    check(ncdhw(dx), xr.grad, dtype, "Conv3Fn stride 2 dgrad")
    check(dw, wr.grad, dtype, "Conv3Fn stride 2 wgrad")
    check(db, dyr.sum((0, 2, 3, 4)), dtype, "Conv3Fn stride 2 bias grad")


# ------------------------------------------------------------------------------------------------------------------
# ConvTranspose k2 s2 / k4 s4
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _deconv_ref(cin, cout, sp, N, k):
    _threads()
    x = ints((N, cin, *sp), cin, 1).requires_grad_(True)
    w = ints((cin, cout, k, k, k), cin, 2).requires_grad_(True)
    b = int_bias(cout, 3)
    y = F.conv_transpose3d(x, w, b, stride=k)
    dy = ints(y.shape, k ** 3 * cout, 4)
    y.backward(dy)
    return dict(x=x.detach(), w=w.detach(), b=b, dy=dy, y=y.detach(), dx=x.grad, dw=w.grad, db=dy.sum((0, 2, 3, 4)))


# second row: the one-child forward slice <24, 1, 1> (fine-voxel index of a lone child) with input gradient <24, 1>; forward
# <3, 3, 2> on a ragged W (a second 16-voxel group holding one voxel); the remaining forward instantiations <6, 2, 2> and <12, 1, 2>.
# Maximum |reference| of the last two (y, dx, dw): 67, 124, 56 and 92, 121, 21
DC2_CASES = [(32, 32, (8, 8, 8), 2), (256, 128, (3, 3, 3), 2), (48, 48, (4, 6, 10), 2), (128, 64, (4, 5, 7), 3),
             (768, 384, (2, 3, 3), 2), (96, 48, (2, 3, 17), 2), (192, 96, (2, 3, 17), 2), (384, 192, (2, 3, 3), 2),
             # Cout = 8: no register or sliced kernel takes it in either dtype, so forward and input gradient run on the generic
             # igemm kernel (csrc/igemm_flat.hip: deconv epilogue on 32-wide blocks, deconv_bwd source on the 16- / 32- / 48-wide block of Cin)
             (16, 8, (2, 3, 5), 2), (32, 8, (2, 3, 5), 2), (48, 8, (2, 3, 5), 2)]


@pytest.mark.parametrize("cin,cout,sp,N,dtype", [(*c, d) for c in DC2_CASES for d in (F32, BF16)])
def test_deconv_k2s2_exact(cin, cout, sp, N, dtype):
    from medicalsemseg_amd import hip
    dev = _dev()
    r = _deconv_ref(cin, cout, sp, N, 2)
    w, b = r["w"].float().to(dev), r["b"].float().to(dev)
    xg, dyg = cl(r["x"], dtype, dev), cl(r["dy"], dtype, dev)
    fine = tuple(2 * v for v in sp)
    dw = torch.full((cin, cout, 2, 2, 2), float("nan"), device=dev)
    with launched() as k:
        y = hip.deconv_k2s2(xg, hip.pack_deconv(w, dtype), b, torch.empty(N, *fine, cout, dtype=dtype, device=dev), cin, cout)
        wpb = hip.pack_deconv(w, dtype, bwd=True)
        dx = hip.deconv_k2s2_bwd_data(dyg, wpb, torch.empty(N, *sp, cin, dtype=dtype, device=dev), cin, cout)
        hip.deconv_k2s2_wgrad(xg, dyg, dw, cin, cout)
    part_ok = hip.deconv_k2s2_small_unit_ok((N, *sp, cin), cin, cout, dtype)
    print(f"deconv_k2s2 {cin}->{cout} @ {sp} N={N} {dtype}: launched {sorted(k.names)}; partial-block input gradient: {part_ok}")
    assert part_ok == (dtype == BF16 and (cin, cout) in ((256, 128), (128, 64), (768, 384), (96, 48), (192, 96), (384, 192)))
    assert "lwg_kernel<deconv>" not in k.names and "igemm_wgrad_kernel<flat>" in k.names   # below 100 k coarse voxels: flat kernel
    if cout == 8:
        assert k.names == {"igemm_fwd_kernel<flat>", "igemm_wgrad_kernel<flat>"} and hip.lib().msseg_cout_block(cin) == cin
    assert_exact(vol(y), r["y"], "deconv_k2s2 fwd")
    assert_exact(vol(dx), r["dx"], "deconv_k2s2 bwd data")
    assert_exact(dw, r["dw"], "deconv_k2s2 wgrad")
    hip.deconv_k2s2_wgrad(xg, dyg, dw, cin, cout, True)
    assert_exact(dw, 2 * r["dw"], "deconv_k2s2 wgrad accumulate")
    db = hip.channel_sum(dyg, torch.empty(cout, device=dev))
    assert_exact(db, r["db"], "deconv_k2s2 bias grad")
    if part_ok:
        part = hip.deconv_k2s2_bwd_partials(dyg, wpb, cin, cout)
        dx2 = hip.conv3d_k3_small_bwd_finish(part, 1, torch.empty(N, *sp, cin, dtype=dtype, device=dev))
        assert_exact(vol(dx2), r["dx"], "deconv_k2s2 bwd partials + finish")


def test_deconv_k2s2_wgrad_one_pass_exact():
    """48 -> 48 on more than 100 k coarse voxels: the weight gradient takes the one-pass kernel with the child-row gather
    (csrc/wgrad_onepass.h, msseg_lwg_deconv_ok); test_deconv_k2s2_exact holds the shapes it rejects"""
    from medicalsemseg_amd import hip
    dev = _dev()
    _threads()
    cin = cout = 48
    N, sp = 2, (40, 41, 32)
    x = ints((N, *sp, cin), N * sp[0] * sp[1] * sp[2], 1)                  # channels-last; the contraction runs over the voxels
    dy = ints((N, *(2 * v for v in sp), cout), N * sp[0] * sp[1] * sp[2], 2)
    ref = torch.einsum("ndhwi,ndahbwco->ioabc", x, dy.view(N, sp[0], 2, sp[1], 2, sp[2], 2, cout))
    xg, dyg = x.to(dev, BF16), dy.to(dev, BF16)
    dw = torch.full((cin, cout, 2, 2, 2), float("nan"), device=dev)
    with launched() as k:
        hip.deconv_k2s2_wgrad(xg, dyg, dw, cin, cout)
    print(f"deconv_k2s2_wgrad 48->48 @ {sp} N={N}: launched {sorted(k.names)}")
    assert k.names == {"lwg_kernel<deconv>"}
    assert_exact(dw, ref, "deconv_k2s2 one-pass wgrad")
    hip.deconv_k2s2_wgrad(xg, dyg, dw, cin, cout, True)
    assert_exact(dw, 2 * ref, "deconv_k2s2 one-pass wgrad accumulate")


# the dc4_* kernels a case must launch (everything else runs on the vector kernels).  48 -> 48 and the square cases on 2 x 3 x 17
# (W = 17: a second W group holding one voxel; 204 coarse voxels: a second 128-voxel chunk with a tail of 76) cover forward
# <1, 2> <2, 2> <2, 3> <3, 2> and weight gradient <8, 2, 4> <12, 3, 4> <8, 4, 2> <6, 6, 1>; 32 -> 48 is forward <1, 3>, whose
# gradients have no MFMA instantiation; 24 -> 40 has none at all
DC4_ALL = "fwd+bwd+wgrad"          # dc4_fwd_kernel, dc4_bwd_kernel, dc4_wgrad_kernel


@pytest.mark.parametrize("cin,cout,sp,dtype,dc4", [(48, 48, (3, 4, 5), BF16, DC4_ALL), (48, 48, (3, 4, 5), F32, "none"),
                                                    (24, 40, (3, 4, 5), BF16, "none"), (24, 40, (3, 4, 5), F32, "none"),
                                                    (32, 32, (2, 3, 17), BF16, DC4_ALL), (64, 64, (2, 3, 17), BF16, DC4_ALL),
                                                    (96, 96, (2, 3, 17), BF16, DC4_ALL), (32, 48, (2, 3, 17), BF16, "fwd")])
def test_deconv_k4s4_exact(cin, cout, sp, dtype, dc4):
    from medicalsemseg_amd import hip
    dev = _dev()
    N = 2
    r = _deconv_ref(cin, cout, sp, N, 4)
    w, b = r["w"].float().to(dev), r["b"].float().to(dev)
    xg, dyg = cl(r["x"], dtype, dev), cl(r["dy"], dtype, dev)
    fine = tuple(4 * v for v in sp)
    dw = torch.full((cin, cout, 4, 4, 4), float("nan"), device=dev)
    with launched() as k:
        y = hip.deconv_k4s4(xg, hip.pack_deconv(w, dtype), b, torch.empty(N, *fine, cout, dtype=dtype, device=dev), cin, cout)
        dx = hip.deconv_k4s4_bwd_data(dyg, hip.pack_deconv(w, dtype, bwd=True), torch.empty(N, *sp, cin, dtype=dtype, device=dev), cin, cout)
        hip.deconv_k4s4_wgrad(xg, dyg, dw, cin, cout)
    print(f"deconv_k4s4 {cin}->{cout} @ {sp} {dtype}: launched {sorted(k.names)}")
    assert {n for n in k.names if n.startswith("dc4_")} == {f"dc4_{v}_kernel" for v in dc4.split("+") if v != "none"}
    assert_exact(vol(y), r["y"], "deconv_k4s4 fwd")
    assert_exact(vol(dx), r["dx"], "deconv_k4s4 bwd data")
    assert_exact(dw, r["dw"], "deconv_k4s4 wgrad")
    hip.deconv_k4s4_wgrad(xg, dyg, dw, cin, cout, True)
    assert_exact(dw, 2 * r["dw"], "deconv_k4s4 wgrad accumulate")
    assert_exact(hip.channel_sum(dyg, torch.empty(cout, device=dev)), r["db"], "deconv_k4s4 bias grad")


# ------------------------------------------------------------------------------------------------------------------
# 1x1x1 conv / Linear
# ------------------------------------------------------------------------------------------------------------------
# (tokens, cin, cout, does the one-pass weight gradient of csrc/linear_wgrad.hip take the shape in bf16?).  Its rule
# (msseg_linear_wgrad_ok): cout / 16 a multiple of 3 and cin / 16 a multiple of 3 (the instantiated slice shapes), and not a few
# tokens (< 1024) against a large weight (cin * cout > 200000).
LIN_CASES = [(17, 1152, 16, False), (433, 1536, 48, True), (54, 3072, 768, False),   # few tokens, deep K: the waves split K (bf16)
             (4099, 48, 144, True),                                                   # many tokens: weights in registers (bf16)
             # Cin of one or four 32-channel k-steps: no register kernel, bf16 too runs csrc/igemm_flat.hip, forward on 48- / 16- /
             # 32-wide cout blocks (the input gradient of the first two has three and two k-steps: register kernel in bf16)
             (301, 32, 48, False), (301, 32, 16, False), (301, 128, 32, False)]


@pytest.mark.parametrize("tokens,cin,cout,lwg,dtype", [(*c, d) for c in LIN_CASES for d in (F32, BF16)])
def test_linear_exact(tokens, cin, cout, lwg, dtype):
    from medicalsemseg_amd import hip
    dev = _dev()
    _threads()
    x, w, b = ints((tokens, cin), cin, 1), ints((cout, cin), cin, 2), int_bias(cout, 3)
    dy = ints((tokens, cout), cout, 4)
    xg, dyg, wg = x.to(dev, dtype), dy.to(dev, dtype), w.float().to(dev)
    one_pass = hip.linear_wgrad_ok(xg, cin, cout)
    with launched() as k:
        y = hip.conv3d_k1(xg, hip.pack_conv_k1(wg, dtype), b.float().to(dev), torch.empty(tokens, cout, dtype=dtype, device=dev), cin, cout)
        dx = hip.conv3d_k1(dyg, hip.pack_conv_k1(wg, dtype, dgrad=True), None, torch.empty(tokens, cin, dtype=dtype, device=dev), cout, cin)
        dw = torch.full((cout, cin), float("nan"), device=dev)
        hip.conv3d_k1_wgrad(xg, dyg, dw, cin, cout)
    print(f"linear {cin}->{cout}, {tokens} tokens, {dtype}: launched {sorted(k.names)}; one-pass wgrad ok: {one_pass}")
    assert one_pass == (lwg and dtype == BF16)
    if tokens == 301:
        assert "igemm_fwd_kernel<flat>" in k.names and hip.lib().msseg_cout_block(cout) == cout
    assert_exact(y, x @ w.t() + b, "conv3d_k1 fwd")
    assert_exact(dx, dy @ w, "conv3d_k1 dgrad")
    assert_exact(dw, dy.t() @ x, "conv3d_k1_wgrad")
    hip.conv3d_k1_wgrad(xg, dyg, dw, cin, cout, True)
    assert_exact(dw, 2 * (dy.t() @ x), "conv3d_k1_wgrad accumulate")
    if one_pass:
        dw2, db2 = torch.full((cout, cin), float("nan"), device=dev), torch.full((cout,), float("nan"), device=dev)
        with launched() as k:
            hip.linear_wgrad(xg, dyg, dw2, db2, cin, cout)
        assert k.names == {"lwg_kernel"}
        assert_exact(dw2, dy.t() @ x, "linear_wgrad dW")
        assert_exact(db2, dy.sum(0), "linear_wgrad db")
        hip.linear_wgrad(xg, dyg, dw2, db2, cin, cout, True, True)
        assert_exact(dw2, 2 * (dy.t() @ x), "linear_wgrad dW accumulate")
        assert_exact(db2, 2 * dy.sum(0), "linear_wgrad db accumulate")


@pytest.mark.parametrize("cin,cout,dtype", [(32, 3, F32), (32, 3, BF16), (64, 4, F32), (64, 4, BF16)])
def test_conv3d_k1_head_widths_exact(cin, cout, dtype):
    """segmentation-head widths through layers.Conv1 with the padded buffers of the networks: streaming head forward, weight
    gradient from the gradient's channel slice, input gradient over the zero-padded 8 channels"""
    from medicalsemseg_amd.layers import Conv1
    dev = _dev()
    _threads()
    N, sp = 2, (6, 10, 12)
    x = ints((N, cin, *sp), cin, 1).requires_grad_(True)
    w = ints((cout, cin, 1, 1, 1), cin, 2).requires_grad_(True)
    b = int_bias(cout, 3)
    yref = F.conv3d(x, w, b)
    dy = ints(yref.shape, cout, 4)
    yref.backward(dy)
    op = Conv1(torch.nn.Parameter(w.detach().float().to(dev)), torch.nn.Parameter(b.float().to(dev)))
    xg = cl(x.detach(), dtype, dev)
    ybuf = torch.zeros(N, *sp, 8, dtype=dtype, device=dev)
    op.fwd(xg, ybuf[..., :cout])
    assert_exact(vol(ybuf[..., :cout]), yref.detach(), "k1 head fwd")
    assert bool((ybuf[..., cout:] == 0).all())
    dybuf = torch.zeros(N, *sp, 8, dtype=dtype, device=dev)
    dybuf[..., :cout] = cl(dy, dtype, dev)
    dx = op.bwd(xg, dybuf, True, dy_channels=8)
    assert_exact(vol(dx), x.grad, "k1 head dgrad")
    assert_exact(op.w.grad, w.grad, "k1 head wgrad")
    assert_exact(op.b.grad, dy.sum((0, 2, 3, 4)), "k1 head bias grad")


# ------------------------------------------------------------------------------------------------------------------
# one-channel stem, gather conv, depthwise conv
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,sp,N", [(32, (10, 13, 21), 3), (48, (9, 14, 35), 2)])
def test_conv3d_stem_exact(cout, sp, N):
    from medicalsemseg_amd import hip
    dev = _dev()
    _threads()
    x = ints((N, 1, *sp), 27, 1)
    w = ints((cout, 1, 3, 3, 3), 27, 2).requires_grad_(True)
    b = int_bias(cout, 3)
    yref = F.conv3d(x, w, b, padding=1)
    dy = ints(yref.shape, 27 * cout, 4)
    yref.backward(dy)
    xg, dyg = cl(x, BF16, dev), cl(dy, BF16, dev)
    wp = hip.pack_conv_gather(w.detach().float().to(dev), BF16)
    y = torch.empty(N, *sp, cout, dtype=BF16, device=dev)
    stats = torch.full((N, cout, 2), float("nan"), device=dev)
    hip.conv3d_stem(xg, wp, b.float().to(dev), y, cout, stats)
    assert_exact(vol(y), yref.detach(), "stem fwd")
    err = _sumsq_err(stats, yref.detach())
    print(f"conv3d_stem 1->{cout} @ {sp} N={N}: fused sum of squares relative error {err:.3e} (gate {SUMSQ_GATES['stem']:.1e})")
    assert err <= SUMSQ_GATES["stem"]
    dw = torch.full((cout, 1, 3, 3, 3), float("nan"), device=dev)
    hip.conv3d_gather_wgrad(xg, dyg, dw, 1, cout, 3, 1, 1)
    assert_exact(dw, w.grad, "stem wgrad")
    hip.conv3d_gather_wgrad(xg, dyg, dw, 1, cout, 3, 1, 1, True)
    assert_exact(dw, 2 * w.grad, "stem wgrad accumulate")


# cout blocks of the gather source (csrc/igemm_flat.hip): 48, 32, 32 and 16 wide
GATHER_CASES = [(1, 48, 2, 2, 0, (12, 12, 12)), (4, 32, 3, 1, 1, (5, 7, 9)), (1, 32, 7, 4, 3, (16, 20, 24)), (4, 16, 3, 1, 1, (5, 7, 9))]


@pytest.mark.parametrize("cin,cout,k,s,p,sp,dtype", [(*c, d) for c in GATHER_CASES for d in (F32, BF16)])
def test_conv3d_gather_exact(cin, cout, k, s, p, sp, dtype):
    from medicalsemseg_amd import hip
    dev = _dev()
    _threads()
    N, K = 2, cin * k ** 3
    x = ints((N, cin, *sp), K, 1)
    w = ints((cout, cin, k, k, k), K, 2).requires_grad_(True)
    b = int_bias(cout, 3)
    yref = F.conv3d(x, w, b, stride=s, padding=p)
    dy = ints(yref.shape, cout, 4)
    yref.backward(dy)
    xg, dyg = cl(x, dtype, dev), cl(dy, dtype, dev)
    wp = hip.pack_conv_gather(w.detach().float().to(dev), dtype)
    with launched() as kn:
        y = hip.conv3d_gather(xg, wp, b.float().to(dev), torch.empty(N, *yref.shape[2:], cout, dtype=dtype, device=dev), cin, cout, k, s, p)
        dw = torch.full((cout, cin, k, k, k), float("nan"), device=dev)
        hip.conv3d_gather_wgrad(xg, dyg, dw, cin, cout, k, s, p)
    print(f"conv3d_gather {cin}->{cout} k{k} s{s} p{p} @ {sp} {dtype}: launched {sorted(kn.names)}")
    assert kn.names == {"igemm_fwd_kernel<flat>", "igemm_wgrad_kernel<flat>"}
    assert_exact(vol(y), yref.detach(), "gather fwd")
    assert_exact(dw, w.grad, "gather wgrad")
    hip.conv3d_gather_wgrad(xg, dyg, dw, cin, cout, k, s, p, True)
    assert_exact(dw, 2 * w.grad, "gather wgrad accumulate")


@pytest.mark.parametrize("C,sp,dtype", [(c, sp, d) for c, sp in ((40, (5, 7, 9)), (192, (6, 6, 6)), (1536, (3, 3, 3))) for d in (F32, BF16)])
def test_dwconv3d_k3_exact(C, sp, dtype):
    """depthwise 3x3x3 through ops.dwconv3: dwconv3d_k3, the same kernel with flip=True as the input gradient, dwconv3d_k3_wgrad"""
    from medicalsemseg_amd import ops
    dev = _dev()
    _threads()
    N = 2
    x = ints((N, C, *sp), 27, 1).requires_grad_(True)
    w = ints((C, 1, 3, 3, 3), 27, 2).requires_grad_(True)
    b = int_bias(C, 3)
    yref = F.conv3d(x, w, b, padding=1, groups=C)
    dy = ints(yref.shape, 27, 4)
    yref.backward(dy)
    wp, bp = torch.nn.Parameter(w.detach().float().to(dev)), torch.nn.Parameter(b.float().to(dev))
    xg = cl(x.detach(), dtype, dev).requires_grad_(True)
    y = ops.dwconv3(xg, wp, bp)
    y.backward(cl(dy, dtype, dev))
    assert_exact(vol(y.detach()), yref.detach(), "dwconv3 fwd")
    assert_exact(vol(xg.grad), x.grad, "dwconv3 dgrad (flip)")
    assert_exact(wp.grad, w.grad, "dwconv3 wgrad")
    assert_exact(bp.grad, dy.sum((0, 2, 3, 4)), "dwconv3 bias grad")
    ops.dwconv3(xg, wp, bp).backward(cl(dy, dtype, dev))
    assert_exact(wp.grad, 2 * w.grad, "dwconv3 wgrad accumulate")
