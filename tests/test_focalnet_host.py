"""CPU-side checks of FocalNetUNETR: the builder surface, parameter count / order / state-dict shapes against the reference
class (tests/golden/param_order_focalnet.json), and the plain-torch restatement tests/focalnet_ref.py against the fixture
the REFERENCE's own FocalNet produced (tools/gen_golden_focalnet.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests.golden_util import det_fill_, det_tensor

CLI = "--model FocalNetUNETR --patch_size 2 --window_size 9 --output_dim 3"
GOLD_CFG = dict(patch_size=(2, 2, 2), in_chans=1, embed_dim=16, depths=(2, 1, 1), focal_windows=(3, 5, 3))


def _build(cli):
    from medicalsemseg_amd.models.model_builder import build_model
    from medicalsemseg_amd.utils.arguments import get_args
    return build_model(get_args(cli.split()))


def test_build_model_constructs_with_reference_parameter_count():
    from medicalsemseg_amd.models.focalnet import FocalNet
    net = _build(CLI)
    assert isinstance(net.encoder, FocalNet) and net.out_channels == 3
    # the reference class at 96^3 / patch 2 / width 48 / depths 2 2 2 2 / windows 9; padded `f` rows count as the reference's
    assert sum(v.numel() for v in net.encoder.state_dict().values()) == 10830792
    ks = [m.kernel_size for m in net.encoder.modules() if isinstance(m, torch.nn.Conv3d) and m.groups > 1]
    assert set(ks) == {(9, 9, 9), (11, 11, 11)} and len(ks) == 16


def test_state_dict_round_trips_reference_shapes():
    from medicalsemseg_amd.models.focalnet import FocalNet
    a = FocalNet((32, 32, 32), **GOLD_CFG)
    sd = a.state_dict()
    f = a.layers[0].blocks[0].modulation.f
    assert tuple(f.weight.shape) == (40, 16) and tuple(f.bias.shape) == (40,)
    assert tuple(sd["layers.0.blocks.0.modulation.f.weight"].shape) == (35, 16)
    assert tuple(sd["layers.0.blocks.0.modulation.f.bias"].shape) == (35,)
    assert tuple(sd["layers.1.blocks.0.modulation.f.weight"].shape) == (67, 32)
    assert bool((f.weight[35:] == 0).all()) and bool((f.bias[35:] == 0).all())
    b = FocalNet((32, 32, 32), **GOLD_CFG)
    b.load_state_dict(sd, strict=True)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n
    assert bool((b.layers[0].blocks[0].modulation.f.weight[35:] == 0).all())


def test_parameter_order_matches_reference_class(golden_dir):
    from medicalsemseg_amd.models.focalnet import FocalNet
    from medicalsemseg_amd.optim import add_weight_decay
    with open(os.path.join(golden_dir, "param_order_focalnet.json")) as fh:
        want = [(n, s) for n, s in json.load(fh)]
    net = FocalNet((32, 32, 32), **GOLD_CFG)
    got = [(n, list(p.shape)) for n, p in net.named_parameters()]
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, s), (_, w) in zip(got, want):
        if ".modulation.f." in n:      # computes zero-padded to a multiple of 8 (state-dict hooks translate)
            assert s == [(w[0] + 7) // 8 * 8] + w[1:], n
        else:
            assert s == w, n
    groups = add_weight_decay(net, 1e-5)
    names = {id(p): n for n, p in net.named_parameters()}
    order = [[names[id(p)] for p in g["params"]] for g in groups]
    wn = [n for n, s in want if len(s) <= 1 or n.endswith(".bias")], [n for n, s in want if not (len(s) <= 1 or n.endswith(".bias"))]
    assert order[0] == wn[0] and order[1] == wn[1]


def _rel_l2(a, b):
    a = a.detach().double().numpy()
    return float(np.sqrt(((a - b) ** 2).sum() / (b.astype(np.float64) ** 2).sum()))


def test_cpu_restatement_vs_reference_golden(golden_dir):
    """tests/focalnet_ref.py (same algorithm, fp32, CPU) against the reference's own class: features rel-L2 < 1e-4,
    gradients < 1e-3"""
    from tests.focalnet_ref import FocalNetRef
    g = np.load(os.path.join(golden_dir, "focalnet_encoder_v32.npz"))
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    m = FocalNetRef((32, 32, 32), **GOLD_CFG)
    det_fill_(m, "focal")
    outs = m((det_tensor("focal_x", (2, 1, 32, 32, 32)), None, None))
    assert len(outs) == 4
    loss = 0
    for i, o in enumerate(outs):
        err = _rel_l2(o, g[f"out{i}"])
        print(f"feature {i}: rel-L2 {err:.3e}")
        assert err < 1e-4, f"feature {i}"
        loss = loss + (o * det_tensor(f"focal_r{i}", o.shape)).sum()
    loss.backward()
    mod0, mod1 = m.layers[0].blocks[0].modulation, m.layers[1].blocks[0].modulation
    for key, p in (("d_focal_k5", mod0.focal_layers[1][0].weight), ("d_f_w", mod0.f.weight), ("d_h_w", mod0.h.weight),
                   ("d_focal_k7", mod1.focal_layers[1][0].weight)):
        err = _rel_l2(p.grad, g[key])
        print(f"{key}: rel-L2 {err:.3e}")
        assert err < 1e-3, key


@pytest.mark.parametrize("cli", ["--model FocalNetUNETR --patch_size 2 --window_size 6",            # even
                                 "--model FocalNetUNETR --patch_size 2 --window_size 8",
                                 "--model FocalNetUNETR --patch_size 2 --window_size 11",           # kernel 13
                                 "--model FocalNetUNETR --patch_size 2 --window_size 9 --depths 2 2 2",
                                 "--model FocalNetUNETR --patch_size 2 --window_size 9 7",           # wrong length
                                 "--model FocalNetUNETR --patch_size 2 --window_size 9 9 9 9 9",
                                 "--model FocalNetUNETR --window_size 9",                           # default patch size 16
                                 "--model GCViTUNETR"])
def test_unimplemented_settings_raise(cli):
    with pytest.raises(NotImplementedError):
        _build(cli)


def test_window_list_per_stage_and_cpu_refusal():
    net = _build("--model FocalNetUNETR --patch_size 2 --window_size 3 5 7 9 --hidden_dim 16 --vol_size 32")
    ks = [m.kernel_size[0] for m in net.encoder.modules() if isinstance(m, torch.nn.Conv3d) and m.groups > 1]
    assert ks == [3, 5, 3, 5, 5, 7, 5, 7, 7, 9, 7, 9, 9, 11, 9, 11]
    with pytest.raises(RuntimeError, match="GPU only"):
        net((torch.zeros(1, 1, 32, 32, 32), None, None))
