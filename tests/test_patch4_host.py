"""Patch size 4 (the nnFormer setting) of the Swin-UNETR family, host side: the models construct with the reference's
state-dict layout, impossible pyramids are refused at construction, and the CPU oracle reproduces the fixture that the
reference's own encoder produced at patch size 4 (tools/gen_golden_patch4.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import swin as osw
from tests.golden_util import det_fill_, det_tensor

P4_ARGS = ["--patch_size", "4", "--vol_size", "96", "--depths", "2", "2", "2", "--num_heads", "3", "6", "12",
           "--window_size", "6", "6", "3", "--qkv_bias", "--output_dim", "3"]


def _cfg(*extra):
    from medicalsemseg_amd.utils.arguments import get_args
    return get_args(list(extra) + P4_ARGS)


def test_build_model_patch4_state_dict_matches_oracle_layout():
    from medicalsemseg_amd.models.model_builder import build_model
    net = build_model(_cfg("--model", "nnFormerUNETR"))
    enc = osw.SwinTransformerNNFormer((96,) * 3, (4, 4, 4), 1, 48, (2, 2, 2), (3, 6, 12), (6, 6, 3))
    ref = osw.SwinUNETRCustom(enc, 1, 3, 48, 4)
    a, b = net.state_dict(), ref.state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(tuple(a[k].shape) == tuple(b[k].shape) for k in a)
    assert tuple(a["unet_decoders.0.transp_conv.conv.weight"].shape) == (48, 48, 4, 4, 4)
    assert tuple(a["encoder.patch_embed.proj.weight"].shape) == (48, 1, 4, 4, 4)
    assert tuple(a["unet_decoders.1.transp_conv.conv.weight"].shape) == (96, 48, 2, 2, 2)
    # named_parameters order = what FlatAdamW's by-position mapping and a checkpoint's optimizer state index
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in ref.named_parameters()]


@pytest.mark.parametrize("model", ["SwinDepth", "SwInception"])
@pytest.mark.parametrize("affine", [False, True])
def test_build_model_patch4_other_encoders(model, affine):
    from medicalsemseg_amd.models.model_builder import build_model
    net = build_model(_cfg("--model", model, *(["--rel_pos_bias_affine"] if affine else [])))
    sd = net.state_dict()
    assert tuple(sd["unet_decoders.0.transp_conv.conv.weight"].shape) == (48, 48, 4, 4, 4)
    assert tuple(sd["encoder.patch_embed.proj.weight"].shape) == (48, 1, 4, 4, 4)


def test_build_model_patch4_with_affine_bias():
    from medicalsemseg_amd.models.model_builder import build_model
    net = build_model(_cfg("--model", "nnFormerUNETR", "--rel_pos_bias_affine"))
    assert any("rel_pos_bias_affine" in k for k in net.state_dict())


def test_patch4_impossible_pyramid_and_anisotropic_patch_are_refused():
    from medicalsemseg_amd.models import swin_unetr as P
    kw = dict(in_chans=1, embed_dim=48, depths=(2, 2, 2, 2), num_heads=(3, 6, 12, 24), window_size=(6, 6, 3, 3))
    enc = P.SwinTransformerNNFormer((96,) * 3, patch_size=(4, 4, 4), **kw)
    with pytest.raises(ValueError, match="at most three stages"):          # 96 / 4 / 2^4 is not a whole number
        P.SwinUNETRCustom(enc, 1, 3, (96,) * 3, 48, (4, 4, 4))
    P.SwinUNETRCustom(P.SwinTransformerNNFormer((128,) * 3, patch_size=(4, 4, 4), **kw), 1, 3, (128,) * 3, 48, (4, 4, 4))   # 128 = 4 * 2^5
    with pytest.raises(NotImplementedError, match="anisotropic"):
        P.SwinTransformerNNFormer((96,) * 3, patch_size=(4, 4, 2), **kw)
    with pytest.raises(NotImplementedError, match="in_chans"):              # 4 * 4^3 = 256 > 128 taps of the gather kernels
        P.SwinTransformerNNFormer((96,) * 3, patch_size=(4, 4, 4), **dict(kw, in_chans=4))
    from medicalsemseg_amd.layers import Deconv2
    with pytest.raises(NotImplementedError):
        Deconv2(torch.zeros(8, 8, 3, 3, 3), None)


def test_oracle_encoder_reproduces_reference_patch4_fixture(golden_dir):
    """the tolerances of tests/test_oracle_golden.py::test_encoder (v20 / v24 fixtures)"""
    g = np.load(os.path.join(golden_dir, "swin_encoder_p4_v48.npz"))
    vol = (48, 48, 48)
    m = osw.SwinTransformerNNFormer(vol, (4, 4, 4), 1, 32, (2, 2), (2, 4), (6, 3))
    det_fill_(m, "enc_p4")
    x = det_tensor("enc_p4_x", (2, 1) + vol)
    outs = m((x, None, None))
    assert len(outs) == 3
    for i, o in enumerate(outs):
        np.testing.assert_allclose(o.detach().numpy(), g[f"out{i}"], rtol=1e-3, atol=1e-4)
    loss = sum((o * det_tensor(f"enc_p4_r{i}", o.shape)).sum() for i, o in enumerate(outs))
    loss.backward()
    np.testing.assert_allclose(m.layers[0].blocks[1].attn.qkv.weight.grad.numpy(), g["d_qkv_w"], rtol=1e-3, atol=2e-2)
    np.testing.assert_allclose(m.patch_embed.proj.weight.grad.numpy(), g["d_proj_w"], rtol=1e-3, atol=2e-2)
    np.testing.assert_allclose(m.patch_embed.proj.bias.grad.numpy(), g["d_proj_b"], rtol=1e-3, atol=2e-2)
