"""Generate ``tests/golden/swin_encoder_p4_v48.npz``: the REFERENCE's own ``SwinTransformerNNFormer`` with
``patch_size=(4, 4, 4)`` (the nnFormer setting), run on the CPU.

Same rules as ``oracle/gen_golden.py`` (whose import shims and ``_save`` this reuses) and ``tools/gen_golden_affine.py``:
the reference's modules are imported from where they lie, evaluated on deterministic inputs / weights
(``tests/golden_util.py``), and only the resulting arrays are stored.

vol 48^3 -> 12^3 tokens, embed_dim 32, depths [2, 2], heads [2, 4], windows [6, 3], batch 2, stochastic depth 0, eval
mode: the three feature maps (32 @ 12^3, 64 @ 6^3, 128 @ 3^3) plus the gradients of ``patch_embed.proj.weight / bias``
and of ``layers[0].blocks[1].attn.qkv.weight`` under ``det_tensor`` cotangents.  About 0.6 MiB: nothing is subsampled.

    python tools/gen_golden_patch4.py            # rewrites tests/golden/swin_encoder_p4_v48.npz
"""
from __future__ import annotations

import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.gen_golden import REF, _install_import_shims, _save  # noqa: E402
from tests.golden_util import det_fill_, det_tensor  # noqa: E402

NAME = "swin_encoder_p4_v48.npz"
VOL = (48, 48, 48)
CFG = dict(patch_size=(4, 4, 4), in_chans=1, embed_dim=32, depths=[2, 2], num_heads=[2, 4], window_size=[6, 3])


def gen_encoder(ref):
    m = ref.SwinTransformerNNFormer(pretrain_img_size=VOL, drop_path_rate=0.0, **CFG)
    m.eval()
    det_fill_(m, "enc_p4")
    x = det_tensor("enc_p4_x", (2, 1) + VOL)
    outs = m((x, None, None))
    assert [tuple(o.shape[1:]) for o in outs] == [(32, 12, 12, 12), (64, 6, 6, 6), (128, 3, 3, 3)]
    loss = sum((o * det_tensor(f"enc_p4_r{i}", o.shape)).sum() for i, o in enumerate(outs))
    loss.backward()
    _save(NAME, d_proj_w=m.patch_embed.proj.weight.grad, d_proj_b=m.patch_embed.proj.bias.grad,
          d_qkv_w=m.layers[0].blocks[1].attn.qkv.weight.grad, **{f"out{i}": o for i, o in enumerate(outs)})
    size = os.path.getsize(os.path.join(REPO, "tests", "golden", NAME))
    assert size < (1 << 20), f"{NAME}: {size} bytes"


def main():
    if not os.path.isdir(REF):
        raise SystemExit(f"the reference tree {REF} is needed to generate the fixture")
    _install_import_shims()
    torch.set_num_threads(8)
    torch.use_deterministic_algorithms(True)
    import models.backbones.swin_nnformer as ref
    gen_encoder(ref)


if __name__ == "__main__":
    main()
