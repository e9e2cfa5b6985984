#!/usr/bin/env python
"""Test-time inference on the files of a Decathlon data list: what ``run_test.py`` does for ``--synthetic`` volumes (build the
model, load ``cfg.resume``, run ``engine.test.test_model``), fed by files.  The section ``--test_section`` of the data list
(``--data_path`` / ``--task`` / ``--json_list``; ``validation`` without such a section: the held-out cases of fold
``--cv_fold``) is dealt to the ranks; every case is loaded, preprocessed on the device,
predicted, mapped back onto its file's grid (``--restore_mode``) and saved before the next one is read.

    python run_predict.py --data_path /data --task Task09_Spleen --model UNet --output_dim 2 --vol_size 96 \
        --t_voxel_spacings --t_voxel_dims 1.5 --t_fixed_ct_intensity --t_crop_foreground_img --t_spatial_pad \
        --resume out/best_model.pth --save_eval_output --output_dir out
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from medicalsemseg_amd import data_device, data_files
from medicalsemseg_amd.engine.test import test_model
from medicalsemseg_amd.models.model_builder import build_model
from medicalsemseg_amd.utils import misc
from medicalsemseg_amd.utils.arguments import get_args


def section_files(json_path, section, seed, cv_max_folds, cv_fold):
    """the cases of a data-list section; "validation" on a data list without that section is the held-out part of fold
    cv_fold of the seeded split, as data_device.dataset_file_lists (run_training.py, run_evaluation.py) resolves it, so that
    a fold's own validation cases can be predicted, and then scored, with Decathlon's dataset.json as it comes"""
    if section == "validation" and not data_files.has_key(json_path, "validation"):
        return data_files.cv_split(data_files.load_datalist(json_path, "training"), seed, cv_max_folds, cv_fold)[1]
    return data_files.load_datalist(json_path, section)


def main(cfg):
    misc.init_distributed_mode(cfg)
    if not torch.cuda.is_available():
        raise SystemExit("run_predict.py needs an MI355X: medicalsemseg_amd has no CPU fallback")
    if cfg.synthetic:
        raise SystemExit("run_predict.py reads files; --synthetic volumes are run_test.py's")
    device = torch.device("cuda", 0 if os.environ.get("MSSEG_BENCH_ONE_DEVICE") else int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    torch.manual_seed(cfg.seed)
    model = build_model(cfg).to(device)
    cfg.eval = True
    misc.load_model(cfg, model)
    js = data_files.datalist_path(cfg.data_path, cfg.task, cfg.json_list)
    files = section_files(js, cfg.test_section, cfg.seed, cfg.cv_max_folds, cfg.cv_fold)
    data_device.check_output_names(files)                        # over all ranks' files, before they are dealt
    mine = data_files.partition(files, misc.get_world_size(), misc.get_rank(), even_divisible=False)
    print(f"{js}: {len(files)} case(s) in \"{cfg.test_section}\", {len(mine)} on this rank")
    test_model(model, data_device.FileCaseLoader(mine, cfg, device), device, cfg)
    if cfg.distributed:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(get_args())
