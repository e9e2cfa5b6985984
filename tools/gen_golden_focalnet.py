"""Generate ``tests/golden/focalnet_encoder_v32.npz`` and ``tests/golden/param_order_focalnet.json``: the REFERENCE's own
``FocalNet`` (``models/backbones/focalnet_3d.py``), run on the CPU.

Same rules as ``oracle/gen_golden.py`` (whose import shims and ``_save`` this reuses) and ``tools/gen_golden_patch4.py``:
the reference's modules are imported from where they lie, evaluated on deterministic inputs / weights
(``tests/golden_util.py``), and only the resulting arrays are stored.

vol 32^3, patch 2 -> 16^3 tokens, embed_dim 16, depths [2, 1, 1], focal windows [3, 5, 3] (depthwise kernels 3/5, 5/7, 3/5),
out_indices (0, 1, 2), stochastic depth 0, eval mode, batch 2: the four feature maps (16 @ 16^3, 32 @ 8^3, 64 @ 4^3,
128 @ 2^3) plus, under ``det_tensor`` cotangents, the gradients of a 5^3 focal kernel on the 16^3 grid, of the ``f`` and ``h``
weights of the first block, and of a 7^3 focal kernel on the 8^3 grid.

    python tools/gen_golden_focalnet.py          # rewrites the two fixtures
"""
from __future__ import annotations

import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.gen_golden import REF, _install_import_shims, _save  # noqa: E402
from tests.golden_util import det_fill_, det_tensor  # noqa: E402

NAME = "focalnet_encoder_v32.npz"
ORDER = "param_order_focalnet.json"
VOL = (32, 32, 32)
CFG = dict(patch_size=(2, 2, 2), in_chans=1, embed_dim=16, depths=[2, 1, 1], focal_windows=[3, 5, 3], focal_levels=[2, 2, 2],
           out_indices=(0, 1, 2))
GRADS = {"d_focal_k5": "layers.0.blocks.0.modulation.focal_layers.1.0.weight",
         "d_f_w": "layers.0.blocks.0.modulation.f.weight",
         "d_h_w": "layers.0.blocks.0.modulation.h.weight",
         "d_focal_k7": "layers.1.blocks.0.modulation.focal_layers.1.0.weight"}


def gen_encoder(ref):
    m = ref.FocalNet(pretrain_img_size=VOL, drop_path_rate=0.0, **CFG)
    m.eval()
    det_fill_(m, "focal")
    x = det_tensor("focal_x", (2, 1) + VOL)
    outs = m((x, None, None))
    assert [tuple(o.shape[1:]) for o in outs] == [(16, 16, 16, 16), (32, 8, 8, 8), (64, 4, 4, 4), (128, 2, 2, 2)]
    loss = sum((o * det_tensor(f"focal_r{i}", o.shape)).sum() for i, o in enumerate(outs))
    loss.backward()
    params = dict(m.named_parameters())
    assert tuple(params[GRADS["d_focal_k5"]].shape[2:]) == (5, 5, 5) and tuple(params[GRADS["d_focal_k7"]].shape[2:]) == (7, 7, 7)
    _save(NAME, **{k: params[n].grad for k, n in GRADS.items()}, **{f"out{i}": o for i, o in enumerate(outs)})
    size = os.path.getsize(os.path.join(REPO, "tests", "golden", NAME))
    assert size < (1 << 20), f"{NAME}: {size} bytes"
    with open(os.path.join(REPO, "tests", "golden", ORDER), "w") as fh:
        json.dump([[n, list(p.shape)] for n, p in m.named_parameters()], fh)
        fh.write("\n")


def main():
    if not os.path.isdir(REF):
        raise SystemExit(f"the reference tree {REF} is needed to generate the fixture")
    _install_import_shims()
    torch.set_num_threads(8)
    torch.use_deterministic_algorithms(True)
    import models.backbones.focalnet_3d as ref
    gen_encoder(ref)


if __name__ == "__main__":
    main()
