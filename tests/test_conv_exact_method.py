"""Why tests/test_gpu_conv_exact.py exists, shown on the CPU with no kernel involved: a result with ONE product missing at ONE
corner voxel fails the exact integer-input comparison, while the same defect on the suite's randn inputs passes the bf16 gate of
tests/test_gpu_kernels.py::check (max |got - ref| / max |ref| < 6e-3).  Fails, too, if assert_exact is ever relaxed into a
tolerance."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_conv_exact import assert_exact, int_bias, ints
from tests.test_gpu_kernels import gen, rnd

CIN, COUT, SP, N = 128, 32, (6, 6, 6), 2


def test_one_dropped_product_fails_exact_and_passes_the_bf16_gate():
    # integer inputs: exact comparison
    x = ints((N, CIN, *SP), 27 * CIN, 1)
    w = ints((COUT, CIN, 3, 3, 3), 27 * CIN, 2)
    ref = F.conv3d(x, w, int_bias(COUT, 3), padding=1)
    assert_exact(ref.clone(), ref, "the reference itself")
    prod = x[0, :, 0, 0, 0].view(1, CIN) * w[:, :, 1, 1, 1]            # [co, ci]: the centre-tap products of the corner voxel
    co, ci = (prod != 0).nonzero()[0].tolist()
    wrong = ref.clone()
    wrong[0, co, 0, 0, 0] -= prod[co, ci]
    assert int((wrong != ref).sum()) == 1
    with pytest.raises(AssertionError, match="1 of .* elements differ.*all on a volume face: True"):
        assert_exact(wrong, ref, "one product dropped")
    # a bf16 result (what the kernels store) with the same defect
    with pytest.raises(AssertionError):
        assert_exact(wrong.to(torch.bfloat16), ref, "one product dropped, stored in bf16")
    # the suite's randn inputs, bf16-rounded: the median such product is far inside the bf16 gate
    xr, wr = rnd(torch.bfloat16, gen(N, CIN, *SP, seed=1), gen(COUT, CIN, 3, 3, 3, seed=2, scale=(CIN * 27) ** -0.5))
    yref = F.conv3d(xr, wr, gen(COUT, seed=3), padding=1)
    prod = (xr[0, :, 0, 0, 0].view(1, CIN) * wr[:, :, 1, 1, 1]).abs()
    med = prod.flatten().sort().values[prod.numel() // 2]
    co, ci = (prod == med).nonzero()[0].tolist()
    delta = float(prod[co, ci])
    assert delta > 0
    assert delta / float(yref.abs().max()) < 6e-3          # test_gpu_kernels.check(dtype=bfloat16) accepts the wrong result
