"""CPU checks of the spacing-conditioned relative position bias (`--rel_pos_bias_affine`): the model builder accepts the
flag for the three Swin encoder families, the parameters carry the reference's names, shapes and order
(tests/golden/param_order_affine.json, from the reference's own classes by tools/gen_golden_affine.py), and a state dict
keyed like the reference's loads strictly."""
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("nnFormerUNETR", "SwinDepth", "SwInception")
ARGS = "--output_dim 2 --vol_size 32 --patch_size 2 --hidden_dim 16 --depths 2 2 --num_heads 1 2 --window_size 4 4 --qkv_bias"


def _cfg(model, extra=""):
    from medicalsemseg_amd.utils.arguments import get_args
    return get_args(f"--model {model} {ARGS} {extra}".split())


@pytest.mark.parametrize("model", MODELS)
def test_build_model_accepts_rel_pos_bias_affine(model):
    from medicalsemseg_amd.models.model_builder import build_model
    net = build_model(_cfg(model, "--rel_pos_bias_affine"))
    attn = net.encoder.layers[0].blocks[1].attn
    assert attn.rel_pos_bias_affine and net.encoder.rel_pos_bias_affine
    assert tuple(attn.rel_pos_bias_affine_emb.shape) == (7 ** 3, 1, 3)
    assert tuple(attn.rel_pos_bias_affine_lin.weight.shape) == (1, 3)
    # without the flag: no extra parameters
    off = build_model(_cfg(model))
    assert not any("rel_pos_bias_affine" in n for n, _ in off.named_parameters())
    n_aff = sum(1 for n, _ in net.named_parameters() if "rel_pos_bias_affine" in n)
    assert n_aff == 3 * 4 and len(list(net.parameters())) == len(list(off.parameters())) + n_aff


def test_parameter_order_matches_reference_classes_with_affine(golden_dir):
    """named_parameters() of the three encoder families with the flag on, against the reference's own classes (what a
    reference checkpoint's AdamW state indexes by position); SwInception's Inception head is zero-padded: names only"""
    from medicalsemseg_amd.models import swin_unetr as P
    with open(os.path.join(golden_dir, "param_order_affine.json")) as fh:
        ref = json.load(fh)
    kw = dict(patch_size=(2, 2, 2), in_chans=1, embed_dim=16, depths=(2, 2), num_heads=(1, 2), window_size=(4, 4),
              rel_pos_bias_affine=True)
    fams = {"swin_nnformer": P.SwinTransformerNNFormer((32,) * 3, **kw), "swindepth": P.SwinDepth((32,) * 3, **kw),
            "swinception": P.SwInception((32,) * 3, **kw)}
    for fam, net in fams.items():
        got = [(n, list(p.shape)) for n, p in net.named_parameters()]
        want = [(n, s) for n, s in ref[fam]]
        assert [n for n, _ in got] == [n for n, _ in want], fam
        assert any("rel_pos_bias_affine_emb" in n for n, _ in want)
        if fam != "swinception":
            assert got == want, fam
        else:
            assert [g for g in got if "rel_pos_bias" in g[0]] == [w for w in want if "rel_pos_bias" in w[0]]


@pytest.mark.parametrize("model", MODELS)
def test_state_dict_with_reference_keys_loads_strict(model):
    """a checkpoint of the reference's model (same keys, the affine ones included) loads with strict=True and lands in the
    affine parameters"""
    from medicalsemseg_amd.models.model_builder import build_model
    net = build_model(_cfg(model, "--rel_pos_bias_affine"))
    sd = net.state_dict()
    keys = [k for k in sd if "rel_pos_bias_affine" in k]
    assert "encoder.layers.1.blocks.0.attn.rel_pos_bias_affine_emb" in keys
    assert "encoder.layers.1.blocks.0.attn.rel_pos_bias_affine_lin.weight" in keys
    assert "encoder.layers.1.blocks.0.attn.rel_pos_bias_affine_lin.bias" in keys
    g = torch.Generator().manual_seed(3)
    for k in keys:
        sd[k] = torch.randn(sd[k].shape, generator=g)
    other = build_model(_cfg(model, "--rel_pos_bias_affine"))
    other.load_state_dict(sd, strict=True)
    for k in keys:
        assert torch.equal(other.state_dict()[k], sd[k]), k
    # a flag-off model refuses the affine keys under strict loading
    with pytest.raises(RuntimeError, match="rel_pos_bias_affine"):
        build_model(_cfg(model)).load_state_dict(sd, strict=True)


@pytest.mark.parametrize("flag", ["--learned_cls_vectors", "--rel_crop_pos_emb", "--abs_pos_emb", "--global_token"])
def test_other_position_flags_still_refused(flag):
    from medicalsemseg_amd.models.model_builder import build_model
    for model in MODELS:
        with pytest.raises(NotImplementedError, match=flag.lstrip("-")):
            build_model(_cfg(model, f"{flag} --rel_pos_bias_affine"))


def test_expand_affine_rows():
    from medicalsemseg_amd import ops
    a = torch.tensor([[1.0, 2.0, 3.0], [-1.0, 0.5, 2.0]])
    assert torch.equal(ops.expand_affine(a, 2), a)
    assert torch.equal(ops.expand_affine(a, 4), a[[0, 0, 1, 1]])
    assert torch.equal(ops.expand_affine(a[:1], 3), a[[0, 0, 0]])
    with pytest.raises(ValueError, match="do not divide"):
        ops.expand_affine(a, 3)
