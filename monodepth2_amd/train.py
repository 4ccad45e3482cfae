"""Train from KITTI on disk: `python -m monodepth2_amd.train --data_path ... `.

Counterpart of the reference's train.py + Trainer.__init__'s data section (trainer.py:
113-139): the split lists are read, the dataset class is chosen by --dataset, a training
and a validation loader are built (loader.BatchLoader over datasets.py, the per-item work
on the GPU) and `Trainer.train` runs the epochs.  Takes the reference's flags
(options.py); the split lists are not shipped: --split_dir names a folder holding
train_files.txt and val_files.txt (default: splits/<split>/ beside the package).

More than one GPU: launch one process per GPU with torch.distributed.run (INTEGRATION.md
§5); each rank builds its own loader shard (`rank::world_size` of the epoch's batches).
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from .datasets import DATASETS, readlines
from .distributed import init_process_group
from .loader import BatchLoader
from .options import MonodepthOptions
from .pack import open_pack
from .trainer import Trainer

_HERE = os.path.dirname(os.path.abspath(__file__))


def split_files(opt):
    """(train lines, val lines) of --split_dir (trainer.py:118-121)."""
    folder = opt.split_dir or os.path.join(_HERE, "splits", opt.split)
    paths = [os.path.join(folder, "{}_files.txt".format(m)) for m in ("train", "val")]
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError(
            "no split list at {}: the split lists are not shipped with this package; pass --split_dir DIR with "
            "DIR/train_files.txt and DIR/val_files.txt (the reference's splits/{}/ folder)".format(
                ", ".join(missing), opt.split))
    return readlines(paths[0]), readlines(paths[1])


def build_loaders(opt, trainer: Trainer):
    if opt.dataset not in DATASETS:
        raise ValueError("--dataset {} cannot be trained from: choose one of {}".format(opt.dataset, sorted(DATASETS)))
    cls = DATASETS[opt.dataset]
    train_lines, val_lines = split_files(opt)
    img_ext = ".png" if opt.png else ".jpg"
    num_scales = len(opt.scales)
    frame_ids = list(trainer.opt.frame_ids)   # with "s" appended under --use_stereo
    common = dict(batch_size=opt.batch_size, shuffle=True, num_workers=opt.num_workers, rank=trainer.rank,
                  world_size=trainer.world_size, device=trainer.device,
                  device_decode=getattr(opt, "device_decode", False), pack=open_pack(opt),
                  device_png=getattr(opt, "device_png", False))
    train_set = cls(opt.data_path, train_lines, opt.height, opt.width, frame_ids, num_scales, is_train=True,
                    img_ext=img_ext, seed=opt.seed)
    # depth_gt feeds the validation monitor only (Trainer.val_step)
    val_set = cls(opt.data_path, val_lines, opt.height, opt.width, frame_ids, num_scales, is_train=False,
                  img_ext=img_ext, seed=opt.seed + 1, load_depth=True)
    train_loader = BatchLoader(train_set, seed=opt.seed, **common)
    val_loader = BatchLoader(val_set, seed=opt.seed + 1, with_depth=val_set.load_depth, **common)
    return train_loader, val_loader


def main(argv: Optional[Sequence[str]] = None) -> Trainer:
    opt = MonodepthOptions().parse(argv)
    split_files(opt)   # a missing list fails here, before any network is built
    rank, local_rank, world = init_process_group()
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    trainer = Trainer(opt, device=device, rank=rank, world_size=world)
    train_loader, val_loader = build_loaders(opt, trainer)
    if rank == 0:
        print("Training model named:\n  ", opt.model_name)
        print("Models and scalars are saved to:\n  ", opt.log_dir)
        print("Using split:\n  ", opt.split_dir or opt.split)
        print("There are {:d} training items and {:d} validation items\n".format(
            len(train_loader.dataset), len(val_loader.dataset)))
    try:
        trainer.train(train_loader, val_loader if len(val_loader) else None)
    finally:
        train_loader.close()
        val_loader.close()
    return trainer


if __name__ == "__main__":
    main()
