#!/usr/bin/env python
"""Training driver with the reference's flow and flags (``/root/reference/run_training.py:27-190``): distributed
init -> seeds -> data -> build_model -> AdamW(+timm-style weight-decay groups) -> cosine schedule with linear warm-up
-> resume -> criterion (--loss_fn) -> epochs of train_one_epoch / run_validation with best-mDice and periodic checkpoints.

Differences: runs on MI355X through ``medicalsemseg_amd`` (no CPU fallback); without ``--synthetic`` the Decathlon
data list under ``--data_path/--task/--json_list`` is read, preprocessed on the GPU and cached in HBM
(``medicalsemseg_amd/data_device.py``), ``--synthetic`` generates volumes instead; logging is stdout + ``log.txt`` JSON lines (tensorboardX / Neptune are not
available here); bf16 compute instead of fp16 autocast, so the GradScaler is a disabled pass-through;
gradients are exchanged with one flat RCCL all-reduce instead of DDP buckets.
"""
from __future__ import annotations

import datetime
import json
import os
import sys
import time

import numpy as np
import torch

from medicalsemseg_amd import parallel
from medicalsemseg_amd.data import SyntheticLoader
from medicalsemseg_amd.engine.train import train_one_epoch
from medicalsemseg_amd.engine.val import run_validation
from medicalsemseg_amd.losses import build_criterion
from medicalsemseg_amd.models.model_builder import build_model
from medicalsemseg_amd.optim import FlatAdamW, LinearWarmupCosineAnnealingLR, add_weight_decay
from medicalsemseg_amd.utils import misc
from medicalsemseg_amd.utils.arguments import get_args, n_label_values


def file_loaders(cfg, device, seed, vol):
    """Decathlon data list -> this rank's training / validation volumes, preprocessed once and cached in HBM
    (the reference's ``data/dataset_builder.py:431-491``; transforms :19-306 as device kernels, MONAI parity unpinned)"""
    from medicalsemseg_amd.data_device import (DeviceDatasetLoader, DeviceVolumeLoader, build_cache, class_crop_config_from_args,
                                               crop_mode, dataset_file_lists, intensity_config_from_args, normalised_zero)
    crop = crop_mode(cfg)
    class_ratios, center_dilation = class_crop_config_from_args(cfg)
    rank, world = misc.get_rank(), misc.get_world_size()
    part_train, part_val, train, val = dataset_file_lists(cfg, rank, world)
    if misc.is_main_process():
        print("Number of files in training cv split: {}".format(len(train)))
        print("Number of files in val cv split: {}".format(len(val)))
    t0 = time.time()
    rec_train, b_train = build_cache(part_train, cfg, device)
    rec_val, b_val = build_cache(part_val, cfg, device)
    torch.cuda.synchronize()
    # every rank reports (print is rank-0-only under data parallelism)
    sys.stdout.write("rank {}: training partition {} file(s) [{}], validation partition {} file(s), cached {} bytes in HBM, "
                     "preprocessed in {:.2f} s\n".format(rank, len(part_train),
                                                         ", ".join(os.path.basename(f["image"]) for f in part_train),
                                                         len(part_val), b_train + b_val, time.time() - t0))
    sys.stdout.flush()
    n_batches = len(part_train) * cfg.t_n_patches_per_image // cfg.n_images_per_batch
    if n_batches < 1:
        raise SystemExit(f"{len(part_train)} file(s) x --t_n_patches_per_image {cfg.t_n_patches_per_image} do not fill one "
                         f"batch of --n_images_per_batch {cfg.n_images_per_batch}")
    loader_train = DeviceDatasetLoader(rec_train, vol, cfg.n_images_per_batch, n_batches, cfg.t_n_patches_per_image, device,
                                       seed=seed, crop=crop, pos=cfg.t_rand_crop_pos_weight or 1.0,
                                       neg=cfg.t_rand_crop_neg_weight or 1.0, flip_prob=cfg.t_flip_prob, rot_prob=cfg.t_rot_prob,
                                       shift_os=cfg.t_intensity_shift_os, shift_prob=cfg.t_intensity_shift_prob,
                                       scale_f=cfg.t_intensity_scale_factors, scale_prob=cfg.t_intensity_scale_prob,
                                       # image_threshold=0 of the reference, on the scale of the cached volume
                                       image_threshold=normalised_zero(cfg),
                                       # rotation + zoom inside the gather; outside the volume lies what the cache pads with
                                       affine_prob=cfg.t_affine_prob, affine_rotate=cfg.t_affine_rotate,
                                       affine_zoom=cfg.t_affine_zoom, affine_pad=normalised_zero(cfg),
                                       # noise, blur, contrast and gamma on the gathered batch
                                       intensity=intensity_config_from_args(cfg),
                                       # on a z-scored cache the reference's `raw image > 0` is the non-zero mask
                                       image_rule="ne" if cfg.t_zscore else "gt",
                                       # crop centres per class, on the class or within a distance of it
                                       class_ratios=class_ratios, center_dilation=center_dilation)
    report_class_candidates(loader_train, rank)
    return loader_train, DeviceVolumeLoader(rec_val)


def report_class_candidates(loader, rank):
    """class-ratio crop: every rank prints the crop-centre candidates per class of each of its volumes"""
    if loader.crop != "class_ratios":
        return
    for rec, counts in zip(loader.vols, loader.class_candidates):
        sys.stdout.write("rank {}: {} crop-centre candidates per class (ratios {}, dilation {}): {}\n".format(
            rank, os.path.basename(str(rec["filename"])), list(loader.class_ratios), loader.center_dilation, counts))
    sys.stdout.flush()


def synthetic_loaders(cfg, device, seed, vol):
    vval = cfg.synthetic_val_size if isinstance(cfg.synthetic_val_size, int) else cfg.synthetic_val_size[0]
    from medicalsemseg_amd.data_device import class_crop_config_from_args
    class_ratios, center_dilation = class_crop_config_from_args(cfg)
    if class_ratios is not None:
        # the class-ratio crop of the dataset path on the one synthetic volume, wrapped in a cache record
        from medicalsemseg_amd.data import sphere_labels
        from medicalsemseg_amd.data_device import DeviceDatasetLoader, intensity_config_from_args
        g = torch.Generator().manual_seed(seed)
        lab = sphere_labels(2 * vol, n_label_values(cfg))
        img = torch.randn(cfg.in_chans, 2 * vol, 2 * vol, 2 * vol, generator=g) + 0.5 * lab[None]
        rec = {"img": img.to(device).contiguous(), "lab": lab.to(device=device, dtype=torch.uint8).contiguous(),
               "affine": np.eye(4), "original_affine": np.eye(4), "filename": "synthetic_volume"}
        loader_train = DeviceDatasetLoader([rec], vol, cfg.n_images_per_batch, cfg.synthetic_steps, 1, device, seed=seed,
                                           crop="class_ratios", flip_prob=cfg.t_flip_prob, rot_prob=cfg.t_rot_prob,
                                           shift_os=cfg.t_intensity_shift_os, shift_prob=cfg.t_intensity_shift_prob,
                                           scale_f=cfg.t_intensity_scale_factors, scale_prob=cfg.t_intensity_scale_prob,
                                           image_threshold=-1e9, affine_prob=cfg.t_affine_prob,
                                           affine_rotate=cfg.t_affine_rotate, affine_zoom=cfg.t_affine_zoom, affine_pad=0.0,
                                           intensity=intensity_config_from_args(cfg), class_ratios=class_ratios,
                                           center_dilation=center_dilation)
        report_class_candidates(loader_train, misc.get_rank())
    elif cfg.t_rand_crop_fgbg:
        # device-side data path: one synthetic "CT" of 2x the patch size cached in HBM, patches cropped
        # (fg / bg centres with the reference's pos : neg odds) and augmented by one gather kernel per batch
        from medicalsemseg_amd.data import sphere_labels
        from medicalsemseg_amd.data_device import DevicePatchLoader, intensity_config_from_args
        g = torch.Generator().manual_seed(seed)
        lab = sphere_labels(2 * vol, n_label_values(cfg))
        img = torch.randn(cfg.in_chans, 2 * vol, 2 * vol, 2 * vol, generator=g) + 0.5 * lab[None]
        loader_train = DevicePatchLoader(img, lab, vol, cfg.n_images_per_batch, cfg.synthetic_steps, device, seed=seed,
                                         pos=cfg.t_rand_crop_pos_weight or 1.0, neg=cfg.t_rand_crop_neg_weight or 1.0,
                                         flip_prob=cfg.t_flip_prob, rot_prob=cfg.t_rot_prob,
                                         shift_os=cfg.t_intensity_shift_os, shift_prob=cfg.t_intensity_shift_prob,
                                         scale_f=cfg.t_intensity_scale_factors, scale_prob=cfg.t_intensity_scale_prob,
                                         image_threshold=-1e9, affine_prob=cfg.t_affine_prob,
                                         affine_rotate=cfg.t_affine_rotate, affine_zoom=cfg.t_affine_zoom, affine_pad=0.0,
                                         intensity=intensity_config_from_args(cfg))
    else:
        loader_train = SyntheticLoader(cfg.synthetic_steps, cfg.n_images_per_batch, vol, cfg.in_chans, n_label_values(cfg), seed)
    loader_val = SyntheticLoader(1, 1, vval, cfg.in_chans, n_label_values(cfg), seed + 7, with_crop_info=False)
    return loader_train, loader_val


def main(cfg):
    misc.init_distributed_mode(cfg)
    if not torch.cuda.is_available():
        raise SystemExit("run_training.py needs an MI355X: medicalsemseg_amd has no CPU fallback "
                         "(the CPU oracle under oracle/ is test infrastructure)")
    # MSSEG_BENCH_ONE_DEVICE: several gloo ranks on one GPU, to rehearse the data-parallel control flow on a 1-GPU box
    device = torch.device("cuda", 0 if os.environ.get("MSSEG_BENCH_ONE_DEVICE") else int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    seed = cfg.seed + misc.get_rank()
    torch.manual_seed(seed)
    np.random.seed(seed)

    vol = cfg.vol_size if isinstance(cfg.vol_size, int) else cfg.vol_size[0]
    if not cfg.synthetic:
        loader_train, loader_val = file_loaders(cfg, device, seed, vol)
    else:
        loader_train, loader_val = synthetic_loaders(cfg, device, seed, vol)

    model = build_model(cfg).to(device)
    if cfg.distributed:
        # /root/reference/run_training.py:83: every BatchNorm uses the statistics of the global batch under data
        # parallelism (SwinDepth / SwInception / SegFormer3D carry BatchNorms; the InstanceNorm models have none)
        n_bn = parallel.convert_sync_batchnorm(model)
        if n_bn and misc.is_main_process():
            print(f"SyncBatchNorm: {n_bn} BatchNorm holder(s) switched to cross-rank statistics")
    print("parameters:", misc.count_parameters(model))
    groups = add_weight_decay(model, cfg.weight_decay)
    optimizer = FlatAdamW(groups, lr=cfg.lr, betas=(0.9, 0.95), eps=1e-6)
    if cfg.distributed:
        # gradient averaging over the ranks, overlapped with the tail of the backward where the model splits it
        optimizer.grad_sync = parallel.GradSync(optimizer, model)
        # identical initial weights on every rank
        torch.distributed.broadcast(optimizer.flat_param, src=0)
    loss_scaler = torch.amp.GradScaler("cuda", enabled=False)
    scheduler = LinearWarmupCosineAnnealingLR(optimizer, warmup_epochs=cfg.warmup_epochs, max_epochs=cfg.epochs)
    misc.load_model(cfg, model, optimizer, loss_scaler, scheduler)
    criterion = build_criterion(cfg)   # --loss_fn DiceCE | Tversky | DiceFocal

    best, best_epoch = 0.0, 0
    start = time.time()
    for epoch in range(cfg.start_epoch, cfg.epochs):
        if cfg.distributed:
            torch.distributed.barrier()
        stats = train_one_epoch(model, loader_train, optimizer, criterion, device, epoch, loss_scaler, cfg)
        if (epoch + 1) % cfg.val_interval == 0 or epoch + 1 == cfg.epochs:
            if cfg.distributed:
                torch.distributed.barrier()
            vstats = run_validation(model, loader_val, criterion, device, epoch, cfg)
            stats.update(vstats)
            if vstats["val/mDice"] > best and cfg.output_dir:
                best, best_epoch = vstats["val/mDice"], epoch
                misc.save_model(cfg, epoch, model, optimizer, loss_scaler, scheduler, filename="best_model.pth")
        if cfg.output_dir and ((epoch + 1) % cfg.save_ckpt_freq == 0 or epoch + 1 == cfg.epochs):
            misc.save_model(cfg, epoch, model, optimizer, loss_scaler, scheduler)
        if cfg.output_dir and misc.is_main_process():
            os.makedirs(cfg.output_dir, exist_ok=True)
            with open(os.path.join(cfg.output_dir, "log.txt"), "a") as f:
                f.write(json.dumps({"epoch": epoch, **{k: float(v) for k, v in stats.items()}}) + "\n")
        scheduler.step()
    print("Training time", str(datetime.timedelta(seconds=int(time.time() - start))), "best val mDice", best, "at", best_epoch)
    if parallel.is_dist():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(get_args())
