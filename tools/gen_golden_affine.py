"""Generate the ``tests/golden/*affine*`` fixtures of the spacing-conditioned relative position bias
(``--rel_pos_bias_affine``) by running the REFERENCE's own modules on the CPU.

Same rules as ``oracle/gen_golden.py`` (whose import shims and ``_save`` this reuses): the reference's modules are
imported from where they lie, evaluated on deterministic inputs / weights (``tests/golden_util.py``), and only the
resulting arrays are stored.  Large activations are kept at every fourth token so that every file stays well under 1 MiB.

The reference's own initialisation makes the affine term small (about 3e-3 on the encoder outputs); ``det_fill_``
values make it large, and every fixture asserts that the term moves its outputs and gradients far past the test gates.

    python tools/gen_golden_affine.py            # rewrites the affine fixtures under tests/golden/
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.gen_golden import REF, _install_import_shims, _save  # noqa: E402
from tests.golden_util import det_fill_, det_tensor  # noqa: E402

# two samples with different spacings, one axis flipped (RAS orientation gives negative diagonal entries)
AFFINE = [[1.5, 0.8, 2.0], [-0.7, 1.25, 3.0]]
TOKEN_STRIDE = 4          # activations of the window-attention fixtures: every fourth token of every window


def _rel(a, b):
    a, b = a.detach().numpy(), b.detach().numpy()
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _moved(name, with_aff, without, floor=0.1):
    """the affine term must move a checked quantity by far more than the loosest (bf16) test gate"""
    r = _rel(with_aff, without)
    assert r > floor, f"{name}: the affine term moves it by only {r:.2e} (relative to max)"
    return r


def gen_window_attention(ref):
    from oracle.swin import shift_region_mask
    aff = torch.tensor(AFFINE)
    for tag, dim, ws, heads in [("h3w6", 48, 6, 3), ("h24w3", 384, 3, 24)]:
        torch.manual_seed(0)
        m = ref.WindowAttention(dim, window_size=(ws,) * 3, num_heads=heads, qkv_bias=True, rel_pos_bias_affine=True)
        det_fill_(m, "attn_aff_" + tag)
        N, nW = ws ** 3, 8
        x = det_tensor("attn_aff_x_" + tag, (2 * nW, N, dim)).requires_grad_(True)      # B_ = 2 samples x 8 windows
        r = det_tensor("attn_aff_r_" + tag, (2 * nW, N, dim))
        mask = shift_region_mask(2 * ws, 2 * ws, 2 * ws, ws, ws // 2)
        prm = [m.relative_position_bias_table, m.rel_pos_bias_affine_emb, m.rel_pos_bias_affine_lin.weight,
               m.rel_pos_bias_affine_lin.bias]
        res, moved = {}, {}
        for mk, msk in (("nomask", None), ("mask", mask)):
            outs = {}
            for a in (aff, None):
                y, _ = m(x, mask=msk, affine=a)
                g = torch.autograd.grad((y * r).sum(), [x] + prm[:1] + (prm[1:] if a is not None else []))
                outs[a is None] = (y, g)
            (y, g), (y0, g0) = outs[False], outs[True]
            moved[mk] = (_moved(f"{tag} y_{mk}", y, y0), _moved(f"{tag} dx_{mk}", g[0], g0[0]),
                         _moved(f"{tag} dtable_{mk}", g[1], g0[1]))
            res.update({f"y_{mk}": y[:, ::TOKEN_STRIDE], f"dx_{mk}": g[0][:, ::TOKEN_STRIDE], f"dtable_{mk}": g[1],
                        f"demb_{mk}": g[2], f"dlin_w_{mk}": g[3], f"dlin_b_{mk}": g[4]})
        print(tag, "affine term moves (y, dx, dtable) by", moved)
        _save(f"swin_attn_affine_{tag}.npz", affine=aff, **res)


def _encoder_run(m, x, aff, rtag):
    """features + the table / emb / lin gradients of the first layer's shifted block (the encoder's input gradient is not
    kept: in this build the volume enters the encoder through a layout kernel, the decoder takes its own copy)"""
    for p in m.parameters():
        p.grad = None
    x = x.clone().requires_grad_(True)
    outs = m((x, None, aff))
    loss = sum((o * det_tensor(f"{rtag}{i}", o.shape)).sum() for i, o in enumerate(outs))
    loss.backward()
    a = m.layers[0].blocks[1].attn
    g = {"d_table": a.relative_position_bias_table.grad}
    if aff is not None:
        g.update(d_emb=a.rel_pos_bias_affine_emb.grad, d_lin_w=a.rel_pos_bias_affine_lin.weight.grad,
                 d_lin_b=a.rel_pos_bias_affine_lin.bias.grad)
    return outs, g


def _encoder_fixture(name, m, x, rtag, extra=None):
    aff = torch.tensor(AFFINE)
    train = m.training
    outs, g = _encoder_run(m, x, aff, rtag)
    out = dict(affine=aff, **g, **{f"out{i}": o for i, o in enumerate(outs)})
    if extra is not None:
        out.update(extra(m))
    # the affine term must matter: the same module (same weights, BatchNorm statistics restored) without it
    state = {k: v.clone() for k, v in m.state_dict().items()}
    outs0, g0 = _encoder_run(m, x, None, rtag)
    m.load_state_dict(state)
    m.train(train)
    # (out0 is the patch embedding, in front of every attention)
    moved = [_moved(f"{name} out{i}", o, o0, 0.02) for i, (o, o0) in enumerate(zip(outs, outs0)) if i > 0]
    moved.append(_moved(f"{name} d_table", g["d_table"], g0["d_table"]))
    print(name, "affine term moves (features 1..., d_table) by", [f"{v:.2e}" for v in moved])
    _save(name, **out)


def gen_encoder(ref):
    vol = (20, 20, 20)       # a 10^3 token grid under window 6: padded windows
    m = ref.SwinTransformerNNFormer(pretrain_img_size=vol, patch_size=(2, 2, 2), in_chans=1, embed_dim=32, depths=[2, 2],
                                    num_heads=[2, 4], window_size=[6, 3], drop_path_rate=0.0, rel_pos_bias_affine=True)
    m.eval()
    det_fill_(m, "enc_aff")
    _encoder_fixture("swin_encoder_affine_v20.npz", m, det_tensor("enc_aff_x", (2, 1) + vol), "enc_aff_r")


def gen_swindepth():
    import models.backbones.swindepth as SD
    vol = (24, 24, 24)
    m = SD.SwinDepth(pretrain_img_size=vol, patch_size=(2, 2, 2), in_chans=1, embed_dim=32, depths=[2, 2],
                     num_heads=[2, 4], window_size=[6, 3], drop_path_rate=0.0, use_learned_cls_vectors=False,
                     out_indices=(0, 1), rel_pos_bias_affine=True)
    det_fill_(m, "sd_aff")
    m.train()
    _encoder_fixture("swindepth_encoder_affine.npz", m, det_tensor("sd_aff_x", (2, 1) + vol), "sd_aff_r")


def gen_swinception():
    import models.backbones.swinception as SI
    vol = (24, 24, 24)
    m = SI.SwInception(pretrain_img_size=vol, patch_size=(2, 2, 2), in_chans=1, embed_dim=32, depths=[2, 2],
                       num_heads=[2, 4], window_size=[6, 3], drop_path_rate=0.0, use_learned_cls_vectors=False,
                       out_indices=(0, 1), rel_pos_bias_affine=True)
    det_fill_(m, "si_aff")
    m.train()
    _encoder_fixture("swinception_encoder_affine.npz", m, det_tensor("si_aff_x", (2, 1) + vol), "si_aff_r")


def gen_param_order(ref):
    """named_parameters() order and shapes of the three encoder families with the flag on (what a reference checkpoint's
    AdamW state indexes by position)"""
    import models.backbones.swindepth as SD
    import models.backbones.swinception as SI
    kw = dict(pretrain_img_size=(32, 32, 32), patch_size=(2, 2, 2), in_chans=1, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
              window_size=[4, 4], rel_pos_bias_affine=True)
    fams = {"swin_nnformer": ref.SwinTransformerNNFormer(**kw),
            "swindepth": SD.SwinDepth(**kw, use_learned_cls_vectors=False, out_indices=(0, 1)),
            "swinception": SI.SwInception(**kw, use_learned_cls_vectors=False, out_indices=(0, 1))}
    out = {k: [[n, list(p.shape)] for n, p in m.named_parameters()] for k, m in fams.items()}
    path = os.path.join(REPO, "tests", "golden", "param_order_affine.json")
    with open(path, "w") as fh:
        json.dump(out, fh)
    print("wrote", path, {k: len(v) for k, v in out.items()})


def main():
    if not os.path.isdir(REF):
        raise SystemExit(f"the reference tree {REF} is needed to generate the fixtures")
    _install_import_shims()
    torch.set_num_threads(8)
    torch.use_deterministic_algorithms(True)   # the gathered tables' gradients (index backward) in a fixed order: bit-reproducible
    import models.backbones.swin_nnformer as ref
    steps = {"attention": lambda: gen_window_attention(ref), "encoder": lambda: gen_encoder(ref),
             "swindepth": gen_swindepth, "swinception": gen_swinception, "param_order": lambda: gen_param_order(ref)}
    for name in (sys.argv[1:] or list(steps)):
        steps[name]()


if __name__ == "__main__":
    main()
