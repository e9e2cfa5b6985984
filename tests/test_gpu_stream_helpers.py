"""The streaming helpers that the models call between the big kernels -- layout transposes, add, axpy_rows, scale_channels,
channel_sum / channel_stats, GELU forward and backward -- each on its own against torch or float64, at the channel counts
and alignments where they switch between their 16-byte and scalar kernels, with every output inside a sentinel-filled
buffer.  Transposes, add and scale_channels round once from an exact fp32 value, so they are compared bit for bit; the
reductions get integer inputs whose every partial sum is exact in fp32."""
import math

import pytest
import torch

from tests.test_gpu_kernels import _dev
from tests.test_gpu_norm_stream import SENTINEL, Guarded, place

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
LAYOUTS = ["dense", "first", "second"]
MANT = {torch.float32: 23, torch.bfloat16: 7}
SP = {1: (1, 1, 1), 7: (1, 1, 7), 105: (3, 5, 7), 1280: (8, 8, 20), 2592: (12, 12, 18)}
PAD = 64


class Flat:
    """a dense tensor of `shape` inside a sentinel-filled 1-D buffer, `lead` elements past the 16-byte aligned position"""

    def __init__(self, shape, dtype, dev, lead=0, sentinel=SENTINEL):
        n = math.prod(shape)
        self.sentinel = sentinel
        self.buf = torch.full((n + 2 * PAD + lead,), sentinel, dtype=dtype, device=dev)
        self.lo, self.hi = PAD + lead, PAD + lead + n
        self.t = self.buf[self.lo:self.hi].view(shape)

    def assert_exact(self, what):
        assert bool((self.buf[:self.lo] == self.sentinel).all()) and bool((self.buf[self.hi:] == self.sentinel).all()), \
            f"{what}: wrote outside its tensor"
        assert not bool((self.buf[self.lo:self.hi] == self.sentinel).any()), f"{what}: left elements unwritten"


def bits(t):
    """the bit patterns of a float tensor (distinguishes the two zeros)"""
    return t.contiguous().cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(bits(got), bits(want)), f"{what}: not bit-equal ({int((bits(got) != bits(want)).sum())} elements differ)"


def half_ulp(ref, dtype):
    """half a unit in the last place of dtype at the (float64) value ref"""
    _, e = torch.frexp(ref.abs().clamp_min(1e-300))        # |ref| = m * 2^e with m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref), e - 2 - MANT[dtype])


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def ints(*shape, seed, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


# ---- layout transposes -------------------------------------------------------------------------------------------------
def _transpose_source(N, C, sp, dtype):
    """NCDHW values with exact bf16 rounding ties of both parities and signs, and both zeros, among random ones"""
    x = randn(N, C, *sp, seed=C) * 3
    special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0,
                            1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20, 2.0 ** -126, 3e38])
    flat = x.view(-1)
    k = min(flat.numel(), special.numel())
    flat[:k] = special[:k]
    flat[-k:] = special[:k]
    return x.to(dtype)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", [1, 3, 20, 32])
@pytest.mark.parametrize("dst_dtype", DTYPES)
@pytest.mark.parametrize("src_dtype", DTYPES)
def test_to_channels_last_and_first(src_dtype, dst_dtype, C, layout):
    from medicalsemseg_amd import hip
    dev = _dev()
    N, sp = 2, (3, 5, 7)
    src = _transpose_source(N, C, sp, src_dtype)
    want_last = src.permute(0, 2, 3, 4, 1).to(dst_dtype)
    out = Guarded(N, sp, C, layout, dst_dtype, dev)
    hip.to_channels_last(src.to(dev), out.t)
    out.assert_exact("to_channels_last")
    assert_bits(out.t, want_last, "to_channels_last")
    # back: a channels-last source (dense or a channel half of wider rows) to dense NCDHW
    src_last = place(src.permute(0, 2, 3, 4, 1).contiguous().to(dev), layout)
    first = Flat((N, C, *sp), dst_dtype, dev)
    hip.to_channels_first(src_last, first.t)
    first.assert_exact("to_channels_first")
    assert_bits(first.t, src.to(dst_dtype), "to_channels_first")
    if src_dtype == dst_dtype == torch.float32:
        back = Flat((N, C, *sp), torch.float32, dev)
        hip.to_channels_first(out.t, back.t)
        assert_bits(back.t, src, "fp32 -> channels last -> channels first")


# ---- add ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows", [1, 105, 1280])
@pytest.mark.parametrize("C", [32, 20, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_add(dtype, C, rows, layout):
    """C = 20 takes the scalar kernel in bf16, C = 3 in both dtypes"""
    from medicalsemseg_amd import hip
    dev = _dev()
    sp = SP[rows]
    a = (randn(1, *sp, C, seed=1) * 3).to(dtype)
    b = (randn(1, *sp, C, seed=2) * 0.7).to(dtype)
    want = (a.float() + b.float()).to(dtype)
    ag, bg = place(a.to(dev), layout), place(b.to(dev), "dense" if layout == "second" else layout)
    y = Guarded(1, sp, C, layout, dtype, dev)
    hip.add(ag, bg, y.t)
    y.assert_exact("add")
    assert_bits(y.t, want, "add")
    assert torch.equal(ag.cpu(), a) and torch.equal(bg.cpu(), b)


# ---- scale_channels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_channels(dtype, C):
    from medicalsemseg_amd import hip
    dev = _dev()
    N, sp = 3, SP[105]
    x = (randn(N, *sp, C, seed=3) * 2).to(dtype)
    s = randn(N, C, seed=4)
    want = (x.float().view(N, -1, C) * s[:, None, :]).to(dtype).view(x.shape)
    y = Guarded(N, sp, C, "dense", dtype, dev)
    hip.scale_channels(x.to(dev), s.to(dev), y.t)
    y.assert_exact("scale_channels")
    assert_bits(y.t, want, "scale_channels")


# ---- axpy_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["a_and_scale", "no_a", "no_scale"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_axpy_rows(dtype, mode):
    """y[n] = a[n] + s[n] * b[n].  Against float64 on the rounded operands: one rounding of the result to its dtype, and
    2^-22 of the terms for the fp32 product and sum in front of it (the product may or may not be fused into the sum)"""
    from medicalsemseg_amd import hip
    dev = _dev()
    N, E = 3, 840
    a = None if mode == "no_a" else (randn(N, E, seed=5) * 2).to(dtype)
    b = randn(N, E, seed=6).to(dtype)
    s = None if mode == "no_scale" else torch.tensor([0.0, 1.0 / 0.9, 1.37])
    sb = b.double() * (1.0 if s is None else s.double()[:, None])
    ref = sb + (0.0 if a is None else a.double())
    y = Flat((N, E), dtype, dev)
    hip.axpy_rows(None if a is None else a.to(dev), b.to(dev), None if s is None else s.to(dev), y.t)
    y.assert_exact("axpy_rows")
    err = (y.t.cpu().double() - ref).abs()
    bound = half_ulp(ref, dtype) + 2.0 ** -22 * ((0.0 if a is None else a.double().abs()) + sb.abs())
    worst = float((err / bound).max())
    assert worst <= 1.0, f"axpy_rows {mode}: error is {worst:.3f} of the bound"


# ---- channel_sum / channel_stats ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", [3, 20, 32, 48, 520])
@pytest.mark.parametrize("rows", [1, 7, 105, 2592])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_sum_and_stats_exact_on_integers(dtype, N, rows, C, layout):
    """integers in [-4, 4] over at most 2^16 rows: every partial sum and sum of squares is an integer below 2^24, so the
    result is exact whatever the order"""
    from medicalsemseg_amd import hip
    dev = _dev()
    sp = SP[rows]
    x = ints(N, *sp, C, seed=C + rows)
    xg = place(x.to(dev, dtype), layout)
    xd = x.double().view(N, -1, C)
    # statistics per sample
    st = Flat((N, C, 2), torch.float32, dev, sentinel=12345.5)
    hip.channel_stats(xg, st.t)
    st.assert_exact("channel_stats")
    want = torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=-1)
    assert torch.equal(st.t.cpu().double(), want), "channel_stats"
    again = hip.channel_stats(xg)
    assert_bits(again, st.t, "channel_stats twice")
    # channel sums over all samples, overwriting and accumulating onto integers
    out = Flat((C,), torch.float32, dev, sentinel=12345.5)
    hip.channel_sum(xg, out.t)
    out.assert_exact("channel_sum")
    assert torch.equal(out.t.cpu().double(), xd.sum((0, 1))), "channel_sum"
    acc = Flat((C,), torch.float32, dev, sentinel=12345.5)
    start = ints(C, seed=9, lo=-100, hi=100)
    acc.t.copy_(start)
    hip.channel_sum(xg, acc.t, accumulate=True)
    acc.assert_exact("channel_sum accumulate")
    assert torch.equal(acc.t.cpu().double(), xd.sum((0, 1)) + start.double()), "channel_sum accumulate"
    twice = torch.empty(C, device=dev)
    hip.channel_sum(xg, twice)
    assert_bits(twice, out.t, "channel_sum twice")
    assert torch.equal(xg.cpu().float(), x)


# ---- GELU --------------------------------------------------------------------------------------------------------------
def _gelu_inputs(n, dtype):
    pool = torch.cat([torch.linspace(-8, 8, 2049), randn(2050, seed=7)])
    x = pool[torch.arange(n) * (pool.numel() // n)]
    return x.to(dtype), randn(n, seed=8).to(dtype)


@pytest.mark.parametrize("n,lead", [(1, 0), (255, 0), (4099, 0), (4096, 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_fwd_and_bwd(dtype, n, lead):
    """exact-erf GELU and its derivative against float64 on the rounded operands; lead = 1: the tensors start one element
    into their buffers and the kernel takes its scalar path"""
    from medicalsemseg_amd import hip
    dev = _dev()
    x, dy = _gelu_inputs(n, dtype)
    xd, dyd = x.double(), dy.double()
    cdf = 0.5 * (1.0 + torch.erf(xd / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * xd * xd) / math.sqrt(2.0 * math.pi)
    xg, dyg = Flat((n,), dtype, dev, lead), Flat((n,), dtype, dev, lead)
    xg.t.copy_(x); dyg.t.copy_(dy)
    for what, ref, scale in (("gelu_fwd", xd * cdf, torch.ones_like(xd)), ("gelu_bwd", dyd * (cdf + xd * pdf), dyd.abs().clamp_min(1.0))):
        out = Flat((n,), dtype, dev, lead)
        if what == "gelu_fwd":
            hip.gelu_fwd(xg.t, out.t)
        else:
            hip.gelu_bwd(xg.t, dyg.t, out.t)
        out.assert_exact(what)
        err = (out.t.cpu().double() - ref).abs()
        bound = half_ulp(ref, dtype) + 2.0 ** -21 * (1.0 + xd.abs()) * scale
        worst = float((err / bound).max())
        print(f"{what} {dtype} n={n} lead={lead}: error / bound {worst:.3f}")
        assert worst <= 1.0, f"{what}: error is {worst:.3f} of the bound"
    assert torch.equal(xg.t.cpu(), x) and torch.equal(dyg.t.cpu(), dy)
