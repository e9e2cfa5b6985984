"""Pins tests/attention_ref.py (the float64 checker of tests/test_gpu_attention_ref.py) before anything trusts it, and shows on
the CPU, with no kernel involved, that the GPU tests tell a subtly wrong kernel from rounding (as tests/test_conv_exact_method.py
does for the convolutions): a kernel that computed one of the wrong VARIANTS of the reference would break the equality of the
routing test or exceed the measured ATTN_GATES of the random-data test."""
import os

import numpy as np
import pytest
import torch

from oracle import swin as O
from oracle import swin_official as OO
from tests.attention_ref import VARIANTS, window_attention_ref
from tests.golden_util import det_fill_, det_tensor
from tests.test_gpu_attention_ref import (ATTN_GATES, BF16, CASES, EXPECT, F32, PATHS, SUITE_CAPS, assert_routing_exact, metrics,
                                          random_inputs, random_ref, random_ref_of, routing_inputs, routing_ref, routing_ref_of)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())


def _block_and_inputs(res, ws, shift, dim=24, heads=3):
    torch.manual_seed(3)
    blk = O.SwinTransformerBlock(dim, res, heads, ws, shift).double()
    det_fill_(blk, "refhost")
    x = det_tensor("refhost_x", (2, res[0] * res[1] * res[2], dim)).double()
    r = det_tensor("refhost_r", (2, res[0] * res[1] * res[2], dim)).double()
    return blk, x, r


@pytest.mark.parametrize("res,ws,shift", [((5, 8, 7), 3, 1), ((7, 5, 9), 4, 2), ((4, 6, 5), 3, 0)])
def test_reference_equals_oracle_block_on_padded_noncubic_grids(res, ws, shift):
    """oracle.swin.SwinTransformerBlock (pad -> roll -> partition -> WindowAttention -> reverse -> roll -> crop, the reference's
    own order, with the qkv Linear INSIDE the attention) against the same block with its attention replaced by
    window_attention_ref on qkv = Linear(norm1(x)) computed outside, float64: y, dx, d table and d qkv.bias, which holds the
    padded tokens' share"""
    blk, x, r = _block_and_inputs(res, ws, shift)
    S, H, W = res
    pad = [-(-L // ws) * ws for L in res]
    assert pad != list(res) and len(set(res)) == 3
    mask = O.shift_region_mask(*pad, ws, ws // 2 if shift == 0 else shift).double()
    xa = x.clone().requires_grad_(True)
    ya = blk(xa, mask)
    ga = torch.autograd.grad((ya * r).sum(), [xa, blk.attn.relative_position_bias_table, blk.attn.qkv.bias])
    xb = x.clone().requires_grad_(True)
    a = blk.attn
    qkv = a.qkv(blk.norm1(xb)).reshape(2, S, H, W, -1)
    out, _, _ = window_attention_ref(qkv, a.qkv.bias, a.relative_position_bias_table, a.num_heads, ws, shift)
    h = xb + a.proj(out.reshape(2, S * H * W, -1))
    yb = h + blk.mlp(blk.norm2(h))
    gb = torch.autograd.grad((yb * r).sum(), [xb, a.relative_position_bias_table, a.qkv.bias])
    assert _rel(yb, ya) < 1e-12
    for u, v, n in zip(gb, ga, ("dx", "dtable", "d qkv.bias")):
        assert _rel(u, v) < 1e-11, n


def test_reference_equals_oracle_window_attention_modules():
    """oracle.swin.WindowAttention on the windows of a shifted grid, and oracle.swin_official.WindowAttention with a clamped
    window under the 7^3 table (MONAI's [:n, :n] slice of the index), float64; lse against logsumexp of the same scores"""
    from oracle.swin import shift_region_mask, window_partition, window_reverse
    torch.manual_seed(5)
    dim, heads, ws, shift, (S, H, W) = 24, 3, 3, 1, (6, 9, 3)
    m = O.WindowAttention(dim, ws, heads).double()
    det_fill_(m, "refhost_wa")
    x = det_tensor("refhost_wa_x", (2, S, H, W, dim)).double()
    xs = torch.roll(x, shifts=(-shift,) * 3, dims=(1, 2, 3))
    want = m(window_partition(xs, ws).reshape(-1, ws ** 3, dim), shift_region_mask(S, H, W, ws, shift).double())
    want = torch.roll(window_reverse(want.reshape(-1, ws, ws, ws, dim), ws, S, H, W), shifts=(shift,) * 3, dims=(1, 2, 3))
    out, lse, pmax = window_attention_ref(m.qkv(x), m.qkv.bias, m.relative_position_bias_table, heads, ws, shift)
    assert _rel(m.proj(out), want) < 1e-12
    assert lse.shape == (2 * (S // ws) * (H // ws) * (W // ws), heads, ws ** 3) and pmax.shape == (2, S, H, W, heads)
    assert float(pmax.min()) > 1.0 / ws ** 3 - 1e-12 and float(pmax.max()) <= 1.0
    # clamped window: 4^3 tokens under the table and index of a 7-window
    mo = OO.WindowAttention(dim, heads, (7, 7, 7)).double()
    det_fill_(mo, "refhost_wo")
    x4 = det_tensor("refhost_wo_x", (2, 4, 4, 4, dim)).double()
    want = mo(x4.reshape(2, 64, dim), None).reshape(2, 4, 4, 4, dim)
    out, lse, _ = window_attention_ref(mo.qkv(x4), mo.qkv.bias, mo.relative_position_bias_table, heads, 4, 0, bias_ws=7)
    assert _rel(mo.proj(out), want) < 1e-12
    sub, _, _ = window_attention_ref(mo.qkv(x4), mo.qkv.bias, mo.relative_position_bias_table, heads, 4, 0, bias_ws=7,
                                     _variant="subcube_index")
    assert _rel(mo.proj(sub), want) > 1e-3                    # the sub-cube index is a different function
    # per-sample tables: sample b under table b alone
    tabs = torch.stack([mo.relative_position_bias_table.detach(), det_tensor("refhost_t1", (13 ** 3, heads), 0.5).double()])
    both, lse2, _ = window_attention_ref(mo.qkv(x4), mo.qkv.bias, tabs, heads, 4, 0, bias_ws=7)
    for b in range(2):
        one, l1, _ = window_attention_ref(mo.qkv(x4[b:b + 1]), mo.qkv.bias, tabs[b], heads, 4, 0, bias_ws=7)
        assert torch.equal(one[0], both[b]) and torch.equal(l1[0], lse2[b])


@pytest.mark.parametrize("tag,dim,ws,heads", [("h3w6", 48, 6, 3), ("h24w3", 384, 3, 24)])
def test_reference_equals_committed_attention_fixtures(tag, dim, ws, heads):
    """tests/golden/swin_attn_*.npz: what the reference project's own WindowAttention computed in fp32 on eight windows of a
    (2 ws)^3 volume, with and without the shift mask.  Gates at fp32 rounding level: y and dx are sums of a few hundred fp32
    products (1e-5 of the maximum); a table entry's gradient sums up to 8 x ws^3 terms that cancel (1e-4)."""
    from oracle.swin import window_partition, window_reverse
    g = np.load(os.path.join(GOLDEN, f"swin_attn_{tag}.npz"))
    m = O.WindowAttention(dim, ws, heads)
    det_fill_(m, "attn_" + tag)
    m = m.double()
    N = ws ** 3
    xw = det_tensor("attn_x_" + tag, (8, N, dim)).double()
    rw = det_tensor("attn_r_" + tag, (8, N, dim)).double()

    def to_volume(t, shift):
        v = window_reverse(t.reshape(8, ws, ws, ws, dim), ws, 2 * ws, 2 * ws, 2 * ws)
        return torch.roll(v, shifts=(shift,) * 3, dims=(1, 2, 3))

    def to_windows(v, shift):
        return window_partition(torch.roll(v, shifts=(-shift,) * 3, dims=(1, 2, 3)), ws).reshape(8, N, dim)

    for mk, shift in (("nomask", 0), ("mask", ws // 2)):
        x = to_volume(xw, shift).requires_grad_(True)
        out, _, _ = window_attention_ref(m.qkv(x), m.qkv.bias, m.relative_position_bias_table, heads, ws, shift)
        y = m.proj(out)
        dx, dt = torch.autograd.grad((y * to_volume(rw, shift)).sum(), [x, m.relative_position_bias_table])
        errs = (_rel(to_windows(y.detach(), shift), torch.from_numpy(g[f"y_{mk}"]).double()),
                _rel(to_windows(dx, shift), torch.from_numpy(g[f"dx_{mk}"]).double()),
                _rel(dt, torch.from_numpy(g[f"dtable_{mk}"]).double()))
        print(f"swin_attn_{tag} {mk}: y {errs[0]:.2e}, dx {errs[1]:.2e}, dtable {errs[2]:.2e}")
        assert errs[0] < 1e-5 and errs[1] < 1e-5 and errs[2] < 1e-4, errs


# ------------------------------------------------------------------------------------------------------------------
# method check: wrong variants of the reference, taken as "what a wrong kernel would return"
# ------------------------------------------------------------------------------------------------------------------
# variant -> (case, the routing equality of (a) breaks, some tensor of (b) exceeds its gate on EVERY path of the case): recorded
# facts, asserted as such.  Every variant is caught at least one way.  The region mask cannot move a one-hot row (the spike wins
# across the -100), so a wrong mask is left to the worst-window gates of (b) and to the averaged rows of (a).
METHOD = {
    "mask_unpadded": ("B", False, True),
    "swap_hw": ("A", True, True),
    "pad_zero": ("A", True, True),
    "subcube_index": ("D", True, True),
    "index_transposed": ("E", True, True),
}


def _over_gates(case, got, ref):
    """on every path of the case, at least one (tensor, metric) of `got` exceeds the gate of the kernel that path runs"""
    (S, H, W), ws, shift, heads, hd, bws = CASES[case]
    caught = []
    for (c, path), (fwd, bwd, _) in EXPECT.items():
        if c != case or PATHS[path][0] != BF16:
            continue
        over = False
        for kernel, name in ((fwd, "out"), (fwd, "lse"), (bwd, "dqkv"), (bwd, "dtable")):
            m = metrics(name, got[name], ref[name], ws, shift)
            g = ATTN_GATES[kernel][name]
            over = over or m[0] > g[0] or m[1] > g[1]
        caught.append(over)
    assert caught
    return all(caught)


def test_gates_are_finite_and_no_looser_than_the_suites():
    for kernel, per in ATTN_GATES.items():
        dtype = F32 if kernel.startswith("fp32") else BF16
        for name, (g1, g2) in per.items():
            assert g1 < float("inf") and g2 < float("inf"), (kernel, name)
            assert g1 <= SUITE_CAPS[dtype].get(name, float("inf")), (kernel, name)


def test_method_table_covers_every_variant():
    assert set(METHOD) == set(VARIANTS)


@pytest.mark.parametrize("variant", VARIANTS)
def test_wrong_variant_of_the_reference_is_caught(variant):
    case, by_equality, by_gates = METHOD[variant]
    ref = routing_ref(case)
    assert_routing_exact(ref["out"].to(torch.bfloat16), ref, "the reference itself")         # and stored in bf16: still equal
    wrong = routing_ref_of(routing_inputs(case), case, _variant=variant)
    try:
        assert_routing_exact(wrong["out"], ref, variant)
        eq_caught = False
    except AssertionError as e:
        eq_caught = True
        assert "exact (token, head) rows differ" in str(e)
    rref = random_ref(case, BF16, False)
    rwrong = random_ref_of(random_inputs(case, BF16, False), case, _variant=variant)
    gates_caught = _over_gates(case, rwrong, rref)
    print(f"{variant} on case {case}: routing equality breaks: {eq_caught}; over the gates of the random-data test: {gates_caught}")
    assert eq_caught or gates_caught
    assert (eq_caught, gates_caught) == (by_equality, by_gates)
